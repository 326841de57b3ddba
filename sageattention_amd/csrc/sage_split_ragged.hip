// sage_split_ragged.hip -- pass 1 of the SPLIT step call (include/sage_kvlsplit_gfx950.h): chunk_max_lens_paged_kernel
// (sage_split_paged.hip) over the DECODE sequences of a step, their query rows packed behind a prefix array.
//
// The ragged sibling of that kernel, in a translation unit of its own so that the kernels there keep their registers: the same Q quantiser and
// row map (cm_quant_q, cm_crow: sage_chunk_max.h), the same MFMA products, integer maxima, one fma per scale group, masks and page lookups, the
// packed (Lq <= 32) grid -- (b, kv head, chunk, block of four heads) -- and the layout of the result, -inf where nothing is visible.  What differs:
//   which sequences take part and where a query row lies -- both from ragged_band (sage_ragged.h) with the band (0, 32]: a sequence outside it
//   leaves without a store; Lq is the sequence's own row count n_b, the offset is clamped with it, row l lies at packed row first_b + l;
//   the row stride of the result -- [B, Hkv, S, group, lq_ws] with lq_ws = min(max_seqlen_q, 32), a quantity of its own
//   (step_split_ws_row, sage_step_list.h); rows n_b .. lq_ws - 1 of a sequence are not written.
// For a decode sequence of n_b rows every value is, bit for bit, what chunk_max_lens_paged_kernel writes for that sample in a call of Lq = n_b.
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_quant_math.h"
#include "sage_chunk_max.h"
#include "sage_ragged.h"
#include "sage_step_list.h"
#include <climits>

namespace sage {

// p: as for launch_chunk_max_lens_paged with Lq = max_seqlen_q and q packed [total_q, Hq, D] (q_sl the row stride, q_sb unused); causal
template <int D, int QDT>
__global__ void __launch_bounds__(256, 2)
chunk_max_lens_ragged_kernel(const ChunkMaxLensParams p, const PagedArgs pa, const RaggedArgs ra, const int lq_ws)
{
    constexpr int KSTEPS = D / 32;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int n = lane & 31, g = lane >> 5;
    const int per_kv = (p.group + 3) >> 2;
    int idx = blockIdx.x;
    const int gi = idx % per_kv;
    idx /= per_kv;
    const int c = idx % p.S;
    idx /= p.S;
    const int hk = idx % p.Hkv, b = idx / p.Hkv;
    const int gq = 4 * gi + wave;
    const int my_row = n;
    // the sequence's rows, if it is a decode sequence: the clamp of every ragged kernel, the band of the step call's decode launch
    int rq0, Lq;
    ragged_band(ra.cu_q[b], ra.cu_q[b + 1], ra.total_q, p.Lq, 0, kStepDecodeRows, rq0, Lq);
    if (gq >= p.group || Lq <= 0) return;       // (waves are independent: no LDS, no barrier)
    const int h = hk * p.group + gq;

    v4i qf[KSTEPS];
    float qsc;
    cm_quant_q<D, QDT>(reinterpret_cast<const uint16_t *>(p.q) + (long)rq0 * p.q_sl + (long)h * p.q_sh + (long)my_row * p.q_sl, my_row < Lq, g, qf, qsc);

    // ---- the sample's length and offset, the chunk's tiles ----
    int len = p.kv_lens[b];
    len = len < 0 ? 0 : (len < p.Lk ? len : p.Lk);
    int s = p.q_start != nullptr ? p.q_start[b] : 0;
    s = s < -Lq ? -Lq : (s < p.Lk ? s : p.Lk);
    int t0, t1;
    step_split_tile_range(c, p.tiles, len, t0, t1);
    {
        const int rlast = 31 < Lq ? 31 : Lq - 1;                          // the wave's last row that exists
        const int vis = s + rlast;                                        // ... and the last key it sees
        const int lim = vis >= 0 ? vis / BLKK + 1 : 0;
        t1 = t1 < lim ? t1 : lim;
    }
    // the page of logical tile t (t0 <= t < t1 <= ceil(len / 64) <= max_pages << page_shift: an entry of the sample's row): wave-uniform index,
    // constant address space -- a scalar load -- and the id clamped on the scalar unit
    typedef const __attribute__((address_space(4))) int *ctable_p;
    const ctable_p row = (ctable_p)pa.block_table + (long)__builtin_amdgcn_readfirstlane(b) * pa.bt_stride;
    const int last_page = pa.num_pages - 1, tmask = (1 << pa.page_shift) - 1;
    auto page_of = [&](int t) -> int {
        const int pg = row[__builtin_amdgcn_readfirstlane(t) >> pa.page_shift];
        return pg < 0 ? 0 : (pg < last_page ? pg : last_page);
    };
    const int8_t *kb = p.k + (long)hk * p.k_sh;
    // lane (n, g) holds bytes 32 kk + 16 g .. + 15 of key rows 32 sb + n of tile t, which lies in page pg
    // (a tile that runs lies in front of ceil(len / 64), so len >= 1 here and rows from len on read row len - 1, a row of the same tile; masked below)
    auto load = [&](int t, int pg, v4i (&kf)[2][KSTEPS]) {
        const int8_t *kt = kb + (long)pg * p.k_sb + (long)((t & tmask) * BLKK) * p.k_sl;
#pragma unroll
        for (int sb = 0; sb < 2; sb++) {
            int key = t * BLKK + sb * 32 + n;
            key = key < len ? key : len - 1;
            const int8_t *kr = kt + (long)(key - t * BLKK) * p.k_sl + 16 * g;
#pragma unroll
            for (int kk = 0; kk < KSTEPS; kk++) kf[sb][kk] = *reinterpret_cast<const v4i *>(kr + 32 * kk);
        }
    };
    int kmax = len - 1;                         // the lane's last visible key (negative: none)
    kmax = kmax < s + my_row ? kmax : s + my_row;
    float mx = -INFINITY;
    v4i kc[2][KSTEPS], kn[2][KSTEPS];
    int pg_c = 0, pg_n = 0;                     // the pages of tile t and of tile t + 1: one lookup per tile
    if (t0 < t1) {
        pg_c = page_of(t0);
        load(t0, pg_c, kc);
    }
    for (int t = t0; t < t1; t++) {
        if (t + 1 < t1) {
            pg_n = page_of(t + 1);
            load(t + 1, pg_n, kn);
        }
        v16i sc[2];
#pragma unroll
        for (int sb = 0; sb < 2; sb++) {
#pragma unroll
            for (int i = 0; i < 16; i++) sc[sb][i] = 0;
#pragma unroll
            for (int kk = 0; kk < KSTEPS; kk++) sc[sb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(kc[sb][kk], qf[kk], sc[sb], 0, 0, 0);
        }
        const float *ksb = p.k_scale + ((long)pg_c * p.Hkv + hk) * p.nks + (t & tmask) * 4;
        const float s0 = ksb[2 * g], s1 = ksb[2 * g + 1];
        const float cs0 = __builtin_ldexpf(p.sm_scale_log2 * (qsc * s0), 26);
        const float cs1 = __builtin_ldexpf(p.sm_scale_log2 * (qsc * s1), 26);
        // (one select per score against the lane's last visible key, no branch: see chunk_max_kernel)
        int m0 = INT_MIN, m1 = INT_MIN;
#pragma unroll
        for (int sb = 0; sb < 2; sb++)
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int key = t * BLKK + sb * 32 + cm_crow(i, g);
                const int v = key <= kmax ? sc[sb][i] : INT_MIN;
                if (i & 2) m1 = max(m1, v);
                else m0 = max(m0, v);
            }
        if (m0 != INT_MIN) mx = fmaxf(mx, __builtin_fmaf(__builtin_ldexpf((float)m0, -26), cs0, -kFp8Offset));
        if (m1 != INT_MIN) mx = fmaxf(mx, __builtin_fmaf(__builtin_ldexpf((float)m1, -26), cs1, -kFp8Offset));
#pragma unroll
        for (int sb = 0; sb < 2; sb++)
#pragma unroll
            for (int kk = 0; kk < KSTEPS; kk++) kc[sb][kk] = kn[sb][kk];
        pg_c = pg_n;
    }
    mx = pair_max(mx);
    if (g == 0 && my_row < Lq) p.out[step_split_ws_row(b, hk, c, gq, my_row, p.Hkv, p.S, p.group, lq_ws)] = mx;
}

// p as for launch_chunk_max_lens_paged, but Lq = max_seqlen_q (any), q packed behind r and the result's row stride lq_ws = min(Lq, 32); causal
hipError_t launch_chunk_max_lens_ragged(const ChunkMaxLensParams &p, const PagedArgs &g, const RaggedArgs &r, int lq_ws, hipStream_t stream)
{
    if (p.Lq <= 0 || p.S <= 0 || p.tiles <= 0 || p.kv_lens == nullptr || p.causal == 0 || r.cu_q == nullptr || r.total_q < 1 ||
        lq_ws != step_split_ws_rows(p.Lq)) return hipErrorInvalidValue;
    if (g.block_table == nullptr || g.page_shift < 0 || g.page_shift > 20 || g.num_pages < 1 || g.max_pages < 1 ||
        (long)p.Lk != ((long)g.max_pages << (6 + g.page_shift)) || p.nks != (4 << g.page_shift)) return hipErrorInvalidValue;
    const long nwg = (long)p.B * p.Hkv * p.S * ((p.group + 3) / 4);
    if (nwg <= 0) return hipSuccess;
    if (nwg > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nwg), block(256);
#define SAGE_CMLR(D_, T_) if (p.D == D_ && p.q_dtype == T_) { hipLaunchKernelGGL((chunk_max_lens_ragged_kernel<D_, T_>), grid, block, 0, stream, p, g, r, lq_ws); return hipGetLastError(); }
    SAGE_CMLR(128, DT_F16) SAGE_CMLR(128, DT_BF16) SAGE_CMLR(64, DT_F16) SAGE_CMLR(64, DT_BF16)
#undef SAGE_CMLR
    return hipErrorInvalidValue;
}

}  // namespace sage
