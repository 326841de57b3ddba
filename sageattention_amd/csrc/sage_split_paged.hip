// sage_split_paged.hip -- pass 1 of the kv_lens family's exact split (num_splits=) over a PAGED cache: the row maximum
// the attention kernel forms over each chunk of a sample's keys, the K rows and their scales reached through a block table.
//
// chunk_max_lens_kernel (sage_split_exact.hip) with other addresses and nothing else: the same Q quantiser (cm_quant_q, sage_chunk_max.h), the same
// MFMA products, integer maxima, one fma per scale group, masks, grid and layout of the result, -inf where nothing is visible.  In a translation
// unit of its own, so that the kernels there keep their registers.  p.k / p.k_scale are the POOL: num_pages pages of 64 << page_shift keys laid out
// as the tensors of a call with B = num_pages (p.k_sb: the page stride, p.Hkv: the pool's kv heads, p.nks = 4 << page_shift: the slots of one
// page); p.Lk is the logical capacity max_pages * page size.  Logical tile t of sample b lies in page
// clamp(block_table[b * bt_stride + (t >> page_shift)], 0, num_pages - 1): one scalar load at a wave-uniform index per tile, clamped before it forms
// an address.  The row clamp `key < len ? key : len - 1` stays inside tile t (a tile that runs lies in front of ceil(len / 64)), so one lookup
// per tile serves its rows and its four scales; only the entries of tiles t0 .. t1 - 1 are read.
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_quant_math.h"
#include "sage_chunk_max.h"
#include <climits>

namespace sage {

template <int D, int QDT, bool CAUSAL>
__global__ void __launch_bounds__(256, 2)
chunk_max_lens_paged_kernel(const ChunkMaxLensParams p, const PagedArgs pa)
{
    constexpr int KSTEPS = D / 32;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int n = lane & 31, g = lane >> 5;
    const bool packed = p.Lq <= 32;
    const int per_kv = packed ? (p.group + 3) >> 2 : p.group;
    int idx = blockIdx.x;
    const int gi = idx % per_kv;
    idx /= per_kv;
    const int c = idx % p.S;
    idx /= p.S;
    const int hk = idx % p.Hkv, b = idx / p.Hkv;
    const int gq = packed ? 4 * gi + wave : gi;
    const int row0 = packed ? 0 : wave * 32, my_row = row0 + n;
    if (gq >= p.group || row0 >= p.Lq) return;  // (waves are independent: no LDS, no barrier)
    const int h = hk * p.group + gq;

    v4i qf[KSTEPS];
    float qsc;
    cm_quant_q<D, QDT>(reinterpret_cast<const uint16_t *>(p.q) + (long)b * p.q_sb + (long)h * p.q_sh + (long)my_row * p.q_sl, my_row < p.Lq, g, qf, qsc);

    // ---- the sample's length and offset, the chunk's tiles ----
    int len = p.kv_lens[b];
    len = len < 0 ? 0 : (len < p.Lk ? len : p.Lk);
    int s = 0;
    if (CAUSAL) {
        s = p.q_start != nullptr ? p.q_start[b] : 0;
        s = s < -p.Lq ? -p.Lq : (s < p.Lk ? s : p.Lk);
    }
    const int t0 = c * p.tiles;
    int t1 = t0 + p.tiles;
    const int nt = (len + BLKK - 1) / BLKK;
    t1 = t1 < nt ? t1 : nt;
    if (CAUSAL) {
        const int rlast = row0 + 31 < p.Lq ? row0 + 31 : p.Lq - 1;      // the wave's last row that exists
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
    if (CAUSAL) kmax = kmax < s + my_row ? kmax : s + my_row;
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
    if (g == 0 && my_row < p.Lq)
        p.out[(((long)b * p.Hkv + hk) * p.S + c) * ((long)p.group * p.Lq) + (long)gq * p.Lq + my_row] = mx;
}

// p as for launch_chunk_max_lens, with k / k_scale / k_sb / Hkv / nks describing the pool (above) and Lk the logical capacity; g: the table
hipError_t launch_chunk_max_lens_paged(const ChunkMaxLensParams &p, const PagedArgs &g, hipStream_t stream)
{
    if (p.Lq > BLKQ || p.Lq <= 0 || p.S <= 0 || p.tiles <= 0 || p.kv_lens == nullptr) return hipErrorInvalidValue;
    if (g.block_table == nullptr || g.page_shift < 0 || g.page_shift > 20 || g.num_pages < 1 || g.max_pages < 1 ||
        (long)p.Lk != ((long)g.max_pages << (6 + g.page_shift)) || p.nks != (4 << g.page_shift)) return hipErrorInvalidValue;
    const long per_kv = p.Lq <= 32 ? (p.group + 3) / 4 : p.group;
    const long nwg = (long)p.B * p.Hkv * p.S * per_kv;
    if (nwg <= 0) return hipSuccess;
    if (nwg > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nwg), block(256);
#define SAGE_CMLP(D_, T_, C_) if (p.D == D_ && p.q_dtype == T_ && (p.causal != 0) == C_) { hipLaunchKernelGGL((chunk_max_lens_paged_kernel<D_, T_, C_>), grid, block, 0, stream, p, g); return hipGetLastError(); }
    SAGE_CMLP(128, DT_F16, false) SAGE_CMLP(128, DT_F16, true) SAGE_CMLP(128, DT_BF16, false) SAGE_CMLP(128, DT_BF16, true)
    SAGE_CMLP(64, DT_F16, false)  SAGE_CMLP(64, DT_F16, true)  SAGE_CMLP(64, DT_BF16, false)  SAGE_CMLP(64, DT_BF16, true)
#undef SAGE_CMLP
    return hipErrorInvalidValue;
}

}  // namespace sage
