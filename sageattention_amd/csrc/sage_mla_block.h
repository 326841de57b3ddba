// sage_mla_block.h -- the per-chunk statistics, their fold and the per-tile quantiser of the absorbed MLA decode route's latent
// (include/sage_mla_gfx950.h), shared by the pre-pass (sage_mla_prepass.hip) and the appendable latent cache (sage_mla_cache.hip), which
// re-forms one 64-key tile with the same operations in the same order and therefore the same bits (as sage_kv_block.h does for D <= 128).
// Device code only; every function is inlined into the kernel that calls it.
#pragma once
#include "sage_mla.h"

namespace sage {

// eight consecutive channels of one row: a 16-byte load, zeros for a row past the last valid one
template <int DT>
__device__ __forceinline__ void mla_load8(const uint16_t *row, bool ok, float (&x)[8])
{
    v4u raw = {0u, 0u, 0u, 0u};
    if (ok) raw = *reinterpret_cast<const v4u *>(row);
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = ld16<DT>((uint16_t)((j & 1) ? (raw[j >> 1] >> 16) : (raw[j >> 1] & 0xffffu)));
}

constexpr int MLA_STATS_THREADS = 576, MLA_STATS_RG = 8, MLA_COLS = MLA_DQK / 8;       // 8 row groups x 72 columns

// ---- statistics ------------------------------------------------------------------------------------------------------------------------
// One 256-token chunk of sample b by 576 threads: the 576 K sums and the 512 maxima of |kv[..., :512]| into the chunk's 1088 workspace floats.
template <int DT>
__device__ __forceinline__ void mla_stats_chunk(const MlaPrepParams &p, int chunk, int b, int tid, float (&red_k)[MLA_STATS_RG][MLA_DQK],
                                                float (&red_v)[MLA_STATS_RG][MLA_DV])
{
    const int kvlen = mla_kv_len(p.kv_lens, b, p.Lk);
    if (chunk * MLA_CHUNK >= kvlen) return;             // (workgroup-uniform) the fold reads the chunks in front of the length only
    const uint16_t *base = reinterpret_cast<const uint16_t *>(p.kv) + (long)b * p.kv_sb;
    const int cl = tid % MLA_COLS, rg = tid / MLA_COLS;
    float sum[8], am[8];
#pragma unroll
    for (int j = 0; j < 8; j++) sum[j] = am[j] = 0.0f;
    for (int i = 0; i < MLA_CHUNK / MLA_STATS_RG; i++) {
        const int tok = chunk * MLA_CHUNK + MLA_STATS_RG * i + rg;
        float x[8];
        mla_load8<DT>(base + (long)tok * p.kv_sl + 8 * cl, tok < kvlen, x);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            sum[j] += x[j];
            am[j] = fmaxf(am[j], fabsf(x[j]));
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        red_k[rg][8 * cl + j] = sum[j];
        if (8 * cl < MLA_DV) red_v[rg][8 * cl + j] = am[j];
    }
    __syncthreads();
    // the row groups in ascending order: one fixed order of additions per channel
    float *w = p.ws + (long)b * mla_ws_per_sample(p.nchunk) + (long)chunk * MLA_WS_PER_CHUNK;
    float s = 0.0f, a = 0.0f;
#pragma unroll
    for (int r = 0; r < MLA_STATS_RG; r++) s += red_k[r][tid];
    w[tid] = s;
    if (tid < MLA_DV) {
#pragma unroll
        for (int r = 0; r < MLA_STATS_RG; r++) a = fmaxf(a, red_v[r][tid]);
        w[MLA_DQK + tid] = a;
    }
}

// The chunks of sample b folded in ascending order by thread = channel: k_mean[b, tid] is written, the V maximum of channel tid (< 512) is
// returned for the caller to publish (0 for the rope channels).
template <int DT>
__device__ __forceinline__ float mla_fold_channel(const MlaPrepParams &p, int b, int tid)
{
    const int kvlen = mla_kv_len(p.kv_lens, b, p.Lk);
    const int nch = (kvlen + MLA_CHUNK - 1) / MLA_CHUNK;
    const float *w = p.ws + (long)b * mla_ws_per_sample(p.nchunk);
    float s = 0.0f;
    for (int c = 0; c < nch; c++) s += w[(long)c * MLA_WS_PER_CHUNK + tid];
    // the reference's mean is the FP32 sum over the rows, rounded to the input dtype (core.py:773); without smooth_k, and for a sample of no
    // rows, nothing is subtracted
    reinterpret_cast<uint16_t *>(p.k_mean)[(long)b * MLA_DQK + tid] = (p.smooth_k && kvlen > 0) ? st16<DT>(s / (float)kvlen) : (uint16_t)0;
    float a = 0.0f;
    if (tid < MLA_DV)
        for (int c = 0; c < nch; c++) a = fmaxf(a, w[(long)c * MLA_WS_PER_CHUNK + MLA_DQK + tid]);
    return a;
}

// ---- one 64-key tile -------------------------------------------------------------------------------------------------------------------
// What the 256 threads of a tile workgroup share in LDS
struct MlaTileLds {
    float mean[MLA_DQK], vrecp[MLA_DV], ramax[BLKK];
    __attribute__((aligned(16))) unsigned char img[MLA_V_TILE_BYTES];
};

// the sample's mean (input dtype) and 448 / amax of its 512 V channels; the caller's __syncthreads() follows
template <int DT>
__device__ __forceinline__ void mla_tile_constants(MlaTileLds &s, const uint16_t *k_mean, const float *v_amax, int tid)
{
    for (int d = tid; d < MLA_DQK; d += 256) s.mean[d] = ld16<DT>(k_mean[d]);
    for (int d = tid; d < MLA_DV; d += 256) {
        const float a = v_amax[d];
        s.vrecp[d] = a > 0.0f ? 448.0f / a : 0.0f;              // (a channel of zeros gives zero bytes, not 0 * inf)
    }
}

// K of one tile: thread = (row r of 64, quarter qd of the row: channels 144 qd .. 144 qd + 143, the image's chunks 9 qd .. 9 qd + 8).
// row_of(r) is row r of the tile (read for r < valid only); the four group scales go to k_scale4, the tile to k_img.  Holds one
// __syncthreads().
template <int DT, class RowOf>
__device__ __forceinline__ void mla_quant_k_tile(MlaTileLds &s, RowOf row_of, int valid, bool smooth_k, unsigned char *k_img, float *k_scale4,
                                                 int tid)
{
    const int r = tid >> 2, qd = tid & 3;
    const bool ok = r < valid;
    const uint16_t *row = row_of(r) + 144 * qd;
    float x[144];
    float amax = 0.0f;
#pragma unroll
    for (int v = 0; v < 18; v++) {
        float f[8];
        mla_load8<DT>(row + 8 * v, ok, f);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            // k - mean in the input dtype (core.py:775), as the reference's quantiser receives it
            const float d = smooth_k ? ld16<DT>(st16<DT>(f[j] - s.mean[144 * qd + 8 * v + j])) : f[j];
            x[8 * v + j] = ok ? d : 0.0f;
            amax = fmaxf(amax, fabsf(x[8 * v + j]));
        }
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    if (qd == 0) s.ramax[r] = amax;
    __syncthreads();
    // per-thread scale groups (quant_per_thread.py:75-83): group j of the tile = rows with (row % 8) / 2 == j
    auto group_scale = [&](int j) {
        float gm = 0.0f;
#pragma unroll
        for (int a = 0; a < 8; a++) gm = fmaxf(gm, fmaxf(s.ramax[8 * a + 2 * j], s.ramax[8 * a + 2 * j + 1]));
        return quant_scale(gm, QS_TRITON_THREAD);
    };
    if (tid < 4) k_scale4[tid] = group_scale(tid);
    const float sc = group_scale((r & 7) >> 1);
    const float y = quant_recip(sc);
#pragma unroll
    for (int c = 0; c < 9; c++) {
        v4u pk;
#pragma unroll
        for (int w4 = 0; w4 < 4; w4++) {
            int q8[4];
#pragma unroll
            for (int j = 0; j < 4; j++) q8[j] = quant_round_triton_nz(x[16 * c + 4 * w4 + j], sc, y);
            pk[w4] = pack_int8x4(q8[0], q8[1], q8[2], q8[3]);
        }
        *reinterpret_cast<v4u *>(k_img + mla_k_offset(r, 9 * qd + c)) = pk;
    }
}

// V of one tile: 64 rows of 64 16-byte loads, e4m3 bytes scattered into the image in LDS (zeros behind the last valid token), the image copied
// out linearly.  SAT clamps to +-448 in front of the conversion (v_cvt_pk_fp8_f32 gives NaN above 464): the pre-pass divides by the maximum of
// the rows it converts and has no value to clamp, the cache's frozen maximum may be exceeded.  Holds one __syncthreads().
template <int DT, bool SAT, class RowOf>
__device__ __forceinline__ void mla_quant_v_tile(MlaTileLds &s, RowOf row_of, int valid, unsigned char *v_img, int tid)
{
#pragma unroll 4
    for (int i = 0; i < 16; i++) {
        const int e = tid + 256 * i, t = e >> 6, cv = e & 63;
        float f[8];
        mla_load8<DT>(row_of(t) + 8 * cv, t < valid, f);
        const int pos = mla_position_of_token(t);
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const int d = 8 * cv + j;
            float a = f[j] * s.vrecp[d], b = f[j + 1] * s.vrecp[d + 1];
            if (SAT) {
                a = fminf(fmaxf(a, -448.0f), 448.0f);
                b = fminf(fmaxf(b, -448.0f), 448.0f);
            }
            const int w2 = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
            s.img[mla_v_offset(d, pos)] = (unsigned char)(w2 & 0xff);
            s.img[mla_v_offset(d + 1, pos)] = (unsigned char)((w2 >> 8) & 0xff);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MLA_V_TILE_BYTES / 4096; i++) {
        const int e = tid + 256 * i;
        *reinterpret_cast<v4u *>(v_img + e * 16) = *reinterpret_cast<const v4u *>(s.img + e * 16);
    }
}

}  // namespace sage
