// sage_mla_split.hip -- the EXACT split of the key range for the absorbed MLA decode call (include/sage_mlasplit_gfx950.h):
// every work item of sage_mla_attn.hip -- (sample, 128-row block of its [Lq * Hq] rows) -- runs as S chunks of T = ceil(ceil(Lk / 64) / S) tiles on
// S times as many workgroups, and every e4m3 P is the P of the unsplit call.  It is the construction of sage_split_exact.hip rebuilt
// for this kernel's work item, image formats and register file: P = exp2(fma(s, c, -m)) is rounded to e4m3 against the RUNNING maximum m, so a
// chunk reproduces the unsplit call's P only if its m starts where the unsplit loop's m stands when it reaches the chunk's first tile.  That
// value is the fmaxf over the earlier chunks' own maxima, so the maxima are formed first.
//
//  * pass 1, mla_chunk_max_kernel<DT>, grid B x nblk x S: chunk_max[b, c, row] = the running maximum the attention loop forms over chunk c's keys
//    alone (-inf where the row sees none).  Q is quantised by the attention prologue's own function (mla_quantise_q), a tile's scores and its
//    maximum are formed by the attention loop's own functions (mla_tile_scores, mla_tile_max: the integer maximum per K-scale group and one fma
//    per group on a tile every row of the wave sees whole, the fma per score behind the mask on a tile that holds a limit), then pair_max, then
//    fmaxf over the chunk's tiles.  The bits agree because the text is shared (sage_mla_loop.h).
//    Its own design: the pass keeps only the 72 Q registers and one tile's 32 scores, so it is built under __launch_bounds__(256, 2), two waves
//    per SIMD, and its ring is K ONLY -- two slots of 36 KiB, 72 KiB per workgroup, V is never touched -- so TWO workgroups share a CU's 160 KiB
//    and one's eighteen-k-step QK^T runs under the other's wait for its tile, which the one-wave attention kernel cannot do.
//    The counted waits: a tile is 36 lane-linear 1-KiB LDS-DMA pieces, NINE per wave, and nothing else of the loop is a vector memory operation
//    (the K scales come by scalar loads, one tile ahead; Q was consumed in the prologue).  Tile t + 1 is requested BEHIND the barrier at the top
//    of tile t, into the slot tile t - 1's QK^T read in front of that barrier.  So at the top of tile t the wave's counted instructions are K of
//    t (9) and nothing younger: vmcnt(0), then the raw barrier (everybody's pieces).  One wait and one barrier per tile.
//  * pass 2, mla_decode_split_kernel<DT> = mla_decode_body<DT, true> of sage_mla_loop.h, grid B x nblk x S: the attention loop of 3.29,
//    unchanged, with the chunk folded into its prologue and m_run seeded from chunk_max; its epilogue stores the FP32 partial O (1 / l) v_scale
//    and log2(l) + m.  The partial goes out as whole rows THROUGH THE FREE RING, 256 channels at a time: the wave's 32-KiB slab holds 32 half
//    rows of 1 KiB, so each store instruction writes one contiguous KiB; straight from the registers it would write 64 pieces of 16 bytes 2 KiB
//    apart.  Same launch bounds and LDS as the unsplit kernel; the compiler's counts are in DESIGN 3.30.
//  * merge, mla_split_merge_kernel<DT>: one thread per (row, 8 channels).  sage_merge.hip's FP32 split merge indexes [B, Hkv, S, group, L] rows
//    and a [B, H, L] LSE; here the rows are [B, S, Lq * Hq] with the LSE transposed to [B, Hq, Lq], so the kernel is this unit's.
#include "../../include/sage_mlasplit_gfx950.h"
#include "sage_mla_loop.h"
#include "sage_host_checks.h"

#include <atomic>

namespace sage {

constexpr int MLA_MAX_LDS_BYTES = 2 * MLA_K_TILE_BYTES;       // pass 1: a two-slot K ring, 72 KiB

template <int DT>
__global__ void __launch_bounds__(256, 2) mla_chunk_max_kernel(const MlaSplitParams pp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MlaAttnParams &p = pp.a;
    constexpr int KSTEPS = MLA_DQK / 32, KTB = MLA_K_TILE_BYTES;
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int n = lane & 31, g = lane >> 5;

    // ---- work item and limits: the expressions of mla_decode_body<DT, true>'s prologue (sage_mla_loop.h) ----
    int item, c;
    mla_split_item(pp, item, c);
    const int tile0 = c * pp.T;
    const int b = item / p.nblk, blk = item % p.nblk;
    const int R = p.rows, Hq = p.Hq, Lq = p.Lq;
    const int kvlen = mla_kv_len(p.kv_lens, b, p.Lk);
    const int shift = kvlen - Lq - tile0 * BLKK;
    const int blk_last = (blk * BLKQ + BLKQ < R ? blk * BLKQ + BLKQ : R) - 1;
    int kend = blk_last / Hq + shift + 1;
    kend = kend < pp.T * BLKK ? kend : pp.T * BLKK;
    float *const cm = pp.chunk_max + ((long)b * pp.S + c) * R;
    if (kend <= 0) {            // (workgroup-uniform) the chunk shows no key to any row of the item: nothing is requested
        if ((int)threadIdx.x <= blk_last - blk * BLKQ) cm[blk * BLKQ + (int)threadIdx.x] = -INFINITY;
        return;
    }
    const int n_tiles = (kend + BLKK - 1) / BLKK;
    const unsigned char *kimg = p.k_img + ((long)b * p.ntile + tile0) * KTB;
    const mla_cfloat_p ks_c = (mla_cfloat_p)(p.k_scale + ((long)b * p.ntile + tile0) * 4);
    mla_issue_tile<MLA_K_PIECES>(kimg, smem, wave, lane);

    const int row0 = blk * BLKQ + wave * 32;
    const int my_row = row0 + n;
    const bool row_ok = my_row < R;
    const int crow = row_ok ? my_row : R - 1;
    const int my_pos = crow / Hq, my_head = crow % Hq;
    const int lim = my_pos + shift;
    const bool wave_ok = row0 < R;
    const int lim_lo = (wave_ok ? row0 / Hq : 0) + shift;
    const int lim_hi = (row0 + 31 < R ? (row0 + 31) / Hq : (R - 1) / Hq) + shift;

    v4i qf[KSTEPS];
    float qsc;
    mla_quantise_q<DT>(reinterpret_cast<const uint16_t *>(p.q) + (long)b * p.q_sb + (long)my_pos * p.q_sl + (long)my_head * p.q_sh, row_ok, g, qf,
                       qsc);
    float ksc0, ksc1;
    mla_k_scales(ks_c, 0, g, ksc0, ksc1);
    const int koff0 = n * 64 + swz_chunk<64>(n, g) * 16, koff1 = n * 64 + swz_chunk<64>(n, 2 + g) * 16;

    float m_chunk = -INFINITY;
    for (int t = 0; t < n_tiles; t++) {
        const int slot = t & 1;
        // vmcnt(0): K of tile t (9) is all the wave has in flight -- the head comment has the count
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        float ksn0 = 0.0f, ksn1 = 0.0f;
        if (t + 1 < n_tiles) {
            mla_issue_tile<MLA_K_PIECES>(kimg + (long)(t + 1) * KTB, smem + (slot ^ 1) * KTB, wave, lane);
            mla_k_scales(ks_c, t + 1, g, ksn0, ksn1);
        }
        const int key0 = t * BLKK;
        if (wave_ok && key0 <= lim_hi) {                        // `active`, as in the attention loop
            v16i s[2];
            mla_tile_scores(smem + slot * KTB, koff0, koff1, qf, s);
            const float cs0 = p.sm_scale_log2 * (qsc * ksc0), cs1 = p.sm_scale_log2 * (qsc * ksc1);
            const bool full = key0 + BLKK - 1 <= lim_lo;
            m_chunk = fmaxf(m_chunk, pair_max(mla_tile_max(s, full, key0, lim, g, cs0, cs1)));
        }
        ksc0 = ksn0;
        ksc1 = ksn1;
    }
    if (g == 0 && row_ok) cm[my_row] = m_chunk;
}

template <int DT>
__global__ void __launch_bounds__(256, 1) mla_decode_split_kernel(const MlaSplitParams pp)
{
    mla_decode_body<DT, true>(pp);
}

// one thread per (row of [B, rows], 8 channels): 64 threads a row, four rows a workgroup
template <int DT>
__global__ void __launch_bounds__(256) mla_split_merge_kernel(const MlaSplitParams pp)
{
    const MlaAttnParams &p = pp.a;
    const long row = (long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int c8 = ((int)threadIdx.x & 63) * 8;
    const long R = p.rows;
    if (row >= (long)p.B * R) return;
    const int b = (int)(row / R), r = (int)(row % R);
    const float *la = pp.lse_part + (long)b * pp.S * R + r;                 // + c * R
    const float *oa = pp.o_part + ((long)b * pp.S * R + r) * MLA_DV + c8;   // + c * R * 512
    float m = -INFINITY;
    for (int c = 0; c < pp.S; c++) m = fmaxf(m, la[(long)c * R]);
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    if (m != -INFINITY)
        for (int c = 0; c < pp.S; c++) {
            const float l = la[(long)c * R];
            if (l == -INFINITY) continue;                                   // the chunk's o_part may hold anything: it is not read
            const float w = __builtin_amdgcn_exp2f(l - m);
            const v4f x0 = *reinterpret_cast<const v4f *>(oa + (long)c * R * MLA_DV), x1 = *reinterpret_cast<const v4f *>(oa + (long)c * R * MLA_DV + 4);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                acc[j] += w * x0[j];
                acc[4 + j] += w * x1[j];
            }
            wsum += w;
        }
    const float inv = wsum > 0.0f ? 1.0f / wsum : 0.0f;
    v4u pk;
#pragma unroll
    for (int w = 0; w < 4; w++) pk[w] = (unsigned)st16<DT>(acc[2 * w] * inv) | ((unsigned)st16<DT>(acc[2 * w + 1] * inv) << 16);
    *reinterpret_cast<v4u *>(reinterpret_cast<uint16_t *>(p.o) + row * MLA_DV + c8) = pk;
    if (p.lse != nullptr && c8 == 0)                                        // row r is position r / Hq, head r % Hq; v_log_f32 is log2
        p.lse[((long)b * p.Hq + r % p.Hq) * p.Lq + r / p.Hq] = wsum > 0.0f ? m + __builtin_amdgcn_logf(wsum) : -INFINITY;
}

static hipError_t launch_mla_split(const MlaSplitParams &pp, int dtype, hipStream_t stream)
{
    const MlaAttnParams &p = pp.a;
    const dim3 grid((unsigned)((long)p.B * p.nblk * pp.S)), mgrid((unsigned)(((long)p.B * p.rows + 3) / 4)), block(256);
    if (dtype == DT_F16) {
        hipLaunchKernelGGL(mla_chunk_max_kernel<DT_F16>, grid, block, MLA_MAX_LDS_BYTES, stream, pp);
        hipLaunchKernelGGL(mla_decode_split_kernel<DT_F16>, grid, block, MLA_LDS_BYTES, stream, pp);
        hipLaunchKernelGGL(mla_split_merge_kernel<DT_F16>, mgrid, block, 0, stream, pp);
    } else {
        hipLaunchKernelGGL(mla_chunk_max_kernel<DT_BF16>, grid, block, MLA_MAX_LDS_BYTES, stream, pp);
        hipLaunchKernelGGL(mla_decode_split_kernel<DT_BF16>, grid, block, MLA_LDS_BYTES, stream, pp);
        hipLaunchKernelGGL(mla_split_merge_kernel<DT_BF16>, mgrid, block, 0, stream, pp);
    }
    return hipGetLastError();
}

static int mlasplit_lds_ready(const char *e)
{
    static std::atomic<unsigned long long> done{0};
    static const void *const kernels[4] = {
        reinterpret_cast<const void *>(&mla_chunk_max_kernel<DT_F16>), reinterpret_cast<const void *>(&mla_chunk_max_kernel<DT_BF16>),
        reinterpret_cast<const void *>(&mla_decode_split_kernel<DT_F16>), reinterpret_cast<const void *>(&mla_decode_split_kernel<DT_BF16>)};
    static const int bytes[4] = {MLA_MAX_LDS_BYTES, MLA_MAX_LDS_BYTES, MLA_LDS_BYTES, MLA_LDS_BYTES};
    return mla_raise_lds(e, done, MLA_LDS_BYTES, kernels, bytes, 4);
}

static int64_t round128(int64_t n) { return (n + 127) / 128 * 128; }

}  // namespace sage

extern "C" {

using namespace sage;

SAGE_MLASPLIT_API int sage_mlasplit_abi_version(void) { return SAGE_MLASPLIT_ABI_VERSION; }

SAGE_MLASPLIT_API int64_t sage_mlasplit_ws_bytes(int B, int Lq, int Hq, int num_splits)
{
    // (B, Lq, Hq < 2^31 and S <= 255: 2052 B S Lq Hq can pass 2^63 only with rows the entry refuses; the bound keeps the product exact)
    if (B < 1 || Lq < 1 || Hq < 1 || num_splits < 2 || num_splits > 255 || (int64_t)Lq * Hq >= ((int64_t)1 << 31))
        return set_last_error(SAGE_EINVAL, "sage_mlasplit_ws_bytes: empty problem or num_splits outside [2, 255] (B %d, Lq %d, Hq %d, num_splits %d)",
                              B, Lq, Hq, num_splits);
    const int64_t n = (int64_t)B * num_splits * ((int64_t)Lq * Hq);
    return 2 * round128(4 * n) + round128(4 * MLA_DV * n);
}

SAGE_MLASPLIT_API int sage_mlasplit_attn(const void *q, const void *k_image, const void *v_image, const float *k_scale, const float *v_scale,
                                         const int32_t *kv_lens, void *o, float *lse, int B, int Lq, int Hq, int Lk, int width_qk, int width_v,
                                         int64_t q_sb, int64_t q_sl, int64_t q_sh, float sm_scale, int dtype, void *stream, int num_splits,
                                         void *ws, int64_t ws_bytes)
{
    const char *const e = "sage_mlasplit_attn";
    MlaSplitParams pp{};
    if (mla_attn_prepare(e, q, k_image, v_image, k_scale, v_scale, kv_lens, o, lse, B, Lq, Hq, Lk, width_qk, width_v, q_sb, q_sl, q_sh, sm_scale,
                         dtype, pp.a) != SAGE_OK)
        return SAGE_EINVAL;
    const int S = num_splits;
    SAGE_REQUIRE(S >= 2 && S <= 255, "%s: num_splits must be in [2, 255] (got %d); call sage_mla_attn for the unsplit call", e, S);
    const int64_t n = (int64_t)B * S * pp.a.rows, seg = round128(4 * n), need = 2 * seg + round128(4 * MLA_DV * n);
    SAGE_REQUIRE(ws != nullptr && (reinterpret_cast<uintptr_t>(ws) & 127u) == 0 && ws_bytes >= need,
                 "%s: ws must be 128-byte aligned and hold sage_mlasplit_ws_bytes(B, Lq, Hq, num_splits) = %lld bytes (got %lld)", e,
                 (long long)need, (long long)ws_bytes);
    SAGE_REQUIRE((int64_t)B * pp.a.nblk * S < ((int64_t)1 << 31) && ((int64_t)B * pp.a.rows + 3) / 4 < ((int64_t)1 << 31),
                 "%s: B * ceil(Lq * Hq / 128) * num_splits and B * Lq * Hq / 4 must be below 2^31", e);
    if (mlasplit_lds_ready(e) != 0) return SAGE_EINVAL;
    pp.S = S;
    pp.T = (pp.a.ntile + S - 1) / S;
    pp.chunk_max = static_cast<float *>(ws);
    pp.lse_part = reinterpret_cast<float *>(static_cast<unsigned char *>(ws) + seg);
    pp.o_part = reinterpret_cast<float *>(static_cast<unsigned char *>(ws) + 2 * seg);
    const hipError_t err = launch_mla_split(pp, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
