// sage_mla_prepass.hip -- the pre-pass of the absorbed multi-head-latent-attention decode route (include/sage_mla_gfx950.h),
// gfx950: one latent [B, Lk, 576] becomes the INT8 K image of all 576 channels and the e4m3 V image of its first 512.
//
// Three launches, no atomics, every grid sized on the host from B and Lk; a sample's valid rows are read from kv_lens on the device, and no row
// from there on is read:
//   1. mla_stats_kernel   one workgroup per 256-token chunk: 576 per-channel K sums and the 512 maxima of |kv[..., :512]| from ONE read of the
//                         latent, 1088 floats per chunk into the workspace.  576 threads = 8 row groups x 72 columns of 8 channels (16-byte
//                         loads); the row groups are folded in ascending order.  A chunk behind the sample's length leaves at once.
//   2. mla_fold_kernel    one workgroup per sample: folds the chunks in ascending order into k_mean [B, 576] (input dtype), v_scale [B, 512] and
//                         the 512 V maxima the quantiser divides by.  A launch of its own: at 64k keys every tile workgroup folding 256 chunks
//                         itself, as the 192 / 128 route does, would re-read a megabyte each.
//   3. mla_quant_kernel   one workgroup per 64-key tile: a K row goes to four threads of 144 channels (nine 16-byte chunks of the image each),
//                         kv - mean in the input dtype, four scales per tile; the 64 x 64 V columns of 8 channels go sixteen to a thread,
//                         scattered as e4m3 bytes into the image in LDS and copied out linearly.  A tile behind the sample's length leaves at once.
// HBM traffic per latent element: read twice (the quantiser's second read of the V channels hits the cache) and written as 1 + 8 / 9 bytes.
#include "../../include/sage_mla_gfx950.h"
#include "sage_mla.h"
#include "sage_host_checks.h"

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

template <int DT>
__global__ void __launch_bounds__(MLA_STATS_THREADS) mla_stats_kernel(const MlaPrepParams p)
{
    __shared__ float red_k[MLA_STATS_RG][MLA_DQK], red_v[MLA_STATS_RG][MLA_DV];
    const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
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

template <int DT>
__global__ void __launch_bounds__(MLA_DQK) mla_fold_kernel(const MlaPrepParams p)
{
    const int b = blockIdx.x, tid = threadIdx.x;        // thread = channel
    const int kvlen = mla_kv_len(p.kv_lens, b, p.Lk);
    const int nch = (kvlen + MLA_CHUNK - 1) / MLA_CHUNK;
    float *w = p.ws + (long)b * mla_ws_per_sample(p.nchunk);
    float s = 0.0f;
    for (int c = 0; c < nch; c++) s += w[(long)c * MLA_WS_PER_CHUNK + tid];
    // the reference's mean is the FP32 sum over the rows, rounded to the input dtype (core.py:773); without smooth_k, and for a sample of no
    // rows, nothing is subtracted
    reinterpret_cast<uint16_t *>(p.k_mean)[(long)b * MLA_DQK + tid] = (p.smooth_k && kvlen > 0) ? st16<DT>(s / (float)kvlen) : (uint16_t)0;
    if (tid < MLA_DV) {
        float a = 0.0f;
        for (int c = 0; c < nch; c++) a = fmaxf(a, w[(long)c * MLA_WS_PER_CHUNK + MLA_DQK + tid]);
        p.v_scale[(long)b * MLA_DV + tid] = a / 448.0f;
        w[(long)p.nchunk * MLA_WS_PER_CHUNK + tid] = a;
    }
}

template <int DT>
__global__ void __launch_bounds__(256) mla_quant_kernel(const MlaPrepParams p)
{
    __shared__ float s_mean[MLA_DQK], s_vrecp[MLA_DV], s_ramax[BLKK];
    __shared__ __attribute__((aligned(16))) unsigned char s_img[MLA_V_TILE_BYTES];
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int kvlen = mla_kv_len(p.kv_lens, b, p.Lk);
    if (tile * BLKK >= kvlen) return;                   // (workgroup-uniform) the attention kernel reads the tiles in front of the length only
    const uint16_t *base = reinterpret_cast<const uint16_t *>(p.kv) + (long)b * p.kv_sb;
    unsigned char *k_img = p.k_img + ((long)b * p.ntile + tile) * MLA_K_TILE_BYTES;
    unsigned char *v_img = p.v_img + ((long)b * p.ntile + tile) * MLA_V_TILE_BYTES;
    const bool smooth_k = p.smooth_k != 0;

    {
        const uint16_t *km = reinterpret_cast<const uint16_t *>(p.k_mean) + (long)b * MLA_DQK;
        const float *va = p.ws + (long)b * mla_ws_per_sample(p.nchunk) + (long)p.nchunk * MLA_WS_PER_CHUNK;
        for (int d = tid; d < MLA_DQK; d += 256) s_mean[d] = ld16<DT>(km[d]);
        for (int d = tid; d < MLA_DV; d += 256) {
            const float a = va[d];
            s_vrecp[d] = a > 0.0f ? 448.0f / a : 0.0f;          // (a channel of zeros gives zero bytes, not 0 * inf)
        }
    }
    __syncthreads();

    // ---- K: thread = (row r of 64, quarter qd of the row: channels 144 qd .. 144 qd + 143, the image's chunks 9 qd .. 9 qd + 8) ----
    {
        const int r = tid >> 2, qd = tid & 3;
        const int key = tile * BLKK + r;
        const bool ok = key < kvlen;
        const uint16_t *row = base + (long)key * p.kv_sl + 144 * qd;
        float x[144];
        float amax = 0.0f;
#pragma unroll
        for (int v = 0; v < 18; v++) {
            float f[8];
            mla_load8<DT>(row + 8 * v, ok, f);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                // k - mean in the input dtype (core.py:775), as the reference's quantiser receives it
                const float d = smooth_k ? ld16<DT>(st16<DT>(f[j] - s_mean[144 * qd + 8 * v + j])) : f[j];
                x[8 * v + j] = ok ? d : 0.0f;
                amax = fmaxf(amax, fabsf(x[8 * v + j]));
            }
        }
        amax = fmaxf(amax, __shfl_xor(amax, 1));
        amax = fmaxf(amax, __shfl_xor(amax, 2));
        if (qd == 0) s_ramax[r] = amax;
        __syncthreads();
        // per-thread scale groups (quant_per_thread.py:75-83): group j of the tile = rows with (row % 8) / 2 == j
        auto group_scale = [&](int j) {
            float gm = 0.0f;
#pragma unroll
            for (int a = 0; a < 8; a++) gm = fmaxf(gm, fmaxf(s_ramax[8 * a + 2 * j], s_ramax[8 * a + 2 * j + 1]));
            return quant_scale(gm, QS_TRITON_THREAD);
        };
        if (tid < 4) p.k_scale[((long)b * p.ntile + tile) * 4 + tid] = group_scale(tid);
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

    // ---- V: 64 rows of 64 16-byte loads, e4m3 bytes scattered into the image in LDS, the image copied out linearly ----
    {
#pragma unroll 4
        for (int i = 0; i < 16; i++) {
            const int e = tid + 256 * i, t = e >> 6, cv = e & 63;
            const int tok = tile * BLKK + t;
            float f[8];
            mla_load8<DT>(base + (long)tok * p.kv_sl + 8 * cv, tok < kvlen, f);
            const int pos = mla_position_of_token(t);
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const int d = 8 * cv + j;
                const int w2 = __builtin_amdgcn_cvt_pk_fp8_f32(f[j] * s_vrecp[d], f[j + 1] * s_vrecp[d + 1], 0, false);
                s_img[mla_v_offset(d, pos)] = (unsigned char)(w2 & 0xff);
                s_img[mla_v_offset(d + 1, pos)] = (unsigned char)((w2 >> 8) & 0xff);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MLA_V_TILE_BYTES / 4096; i++) {
            const int e = tid + 256 * i;
            *reinterpret_cast<v4u *>(v_img + e * 16) = *reinterpret_cast<const v4u *>(s_img + e * 16);
        }
    }
}

hipError_t launch_mla_prepass(const MlaPrepParams &p, int dtype, hipStream_t stream)
{
    const dim3 g1(p.nchunk, p.B), g2(p.B), g3(p.ntile, p.B);
    if (dtype == DT_F16) {
        hipLaunchKernelGGL(mla_stats_kernel<DT_F16>, g1, dim3(MLA_STATS_THREADS), 0, stream, p);
        hipLaunchKernelGGL(mla_fold_kernel<DT_F16>, g2, dim3(MLA_DQK), 0, stream, p);
        hipLaunchKernelGGL(mla_quant_kernel<DT_F16>, g3, dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(mla_stats_kernel<DT_BF16>, g1, dim3(MLA_STATS_THREADS), 0, stream, p);
        hipLaunchKernelGGL(mla_fold_kernel<DT_BF16>, g2, dim3(MLA_DQK), 0, stream, p);
        hipLaunchKernelGGL(mla_quant_kernel<DT_BF16>, g3, dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace sage

extern "C" {

using namespace sage;

SAGE_MLA_API int64_t sage_mla_ws_floats(int B, int Lk)
{
    if (B < 1 || Lk < 1) return set_last_error(SAGE_EINVAL, "sage_mla_ws_floats: empty problem (B %d, Lk %d)", B, Lk);
    return (int64_t)B * mla_ws_per_sample((Lk + MLA_CHUNK - 1) / MLA_CHUNK);
}

SAGE_MLA_API int sage_mla_prepass(const void *kv, const int32_t *kv_lens, void *k_image, float *k_scale, void *k_mean, void *v_image,
                                  float *v_scale, float *ws, int64_t ws_floats, int B, int Lk, int width_qk, int width_v,
                                  int64_t kv_sb, int64_t kv_sl, int smooth_k, int dtype, void *stream)
{
    const char *const e = "sage_mla_prepass";
    SAGE_REQUIRE(width_qk == MLA_DQK && width_v == MLA_DV,
                 "%s: width_qk must be 576 and width_v 512 (got %d and %d); call sage_qk192_prepass for 192 / 128, sage_hd256_prepass for one head_dim up to 256, sage_prepass_kv for 64 / 128",
                 e, width_qk, width_v);
    SAGE_REQUIRE(dtype == DT_F16 || dtype == DT_BF16, "%s: dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got %d)", e, dtype);
    SAGE_REQUIRE(B >= 1 && Lk >= 1, "%s: empty problem (B %d, Lk %d)", e, B, Lk);
    SAGE_REQUIRE(kv && k_image && k_scale && k_mean && v_image && v_scale && ws, "%s: null pointer (only kv_lens may be null)", e);
    SAGE_REQUIRE(aligned16_strides(kv, 8, kv_sb, kv_sl) && kv_sb >= 0 && kv_sl >= MLA_DQK,
                 "%s: kv must be 16-byte aligned with non-negative strides in multiples of 8 elements and a token stride of at least 576", e);
    SAGE_REQUIRE(aligned16(k_image) && aligned16(v_image) && aligned4(k_scale) && aligned4(v_scale) && aligned4(ws) && aligned4(kv_lens) &&
                     (reinterpret_cast<uintptr_t>(k_mean) & 1u) == 0,
                 "%s: the images must be 16-byte aligned, k_scale, v_scale, ws and kv_lens 4-byte, k_mean 2-byte", e);
    const int64_t need = sage_mla_ws_floats(B, Lk);
    SAGE_REQUIRE(ws_floats >= need, "%s: ws holds %lld floats, sage_mla_ws_floats(B, Lk) = %lld", e, (long long)ws_floats, (long long)need);
    SAGE_REQUIRE(B <= 65535, "%s: B must be at most 65535 (got %d)", e, B);
    MlaPrepParams p{};
    p.kv = kv; p.kv_lens = kv_lens;
    p.k_img = static_cast<unsigned char *>(k_image); p.v_img = static_cast<unsigned char *>(v_image);
    p.k_scale = k_scale; p.v_scale = v_scale; p.ws = ws; p.k_mean = k_mean;
    p.kv_sb = kv_sb; p.kv_sl = kv_sl;
    p.B = B; p.Lk = Lk; p.ntile = (Lk + BLKK - 1) / BLKK; p.nchunk = (Lk + MLA_CHUNK - 1) / MLA_CHUNK; p.smooth_k = smooth_k != 0;
    const hipError_t err = launch_mla_prepass(p, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
