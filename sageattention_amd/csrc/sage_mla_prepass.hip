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
// The arithmetic of all three lives in sage_mla_block.h, which the appendable latent cache (sage_mla_cache.hip) calls too.
#include "../../include/sage_mla_gfx950.h"
#include "sage_mla.h"
#include "sage_mla_block.h"
#include "sage_host_checks.h"

namespace sage {

template <int DT>
__global__ void __launch_bounds__(MLA_STATS_THREADS) mla_stats_kernel(const MlaPrepParams p)
{
    __shared__ float red_k[MLA_STATS_RG][MLA_DQK], red_v[MLA_STATS_RG][MLA_DV];
    mla_stats_chunk<DT>(p, blockIdx.x, blockIdx.y, threadIdx.x, red_k, red_v);
}

template <int DT>
__global__ void __launch_bounds__(MLA_DQK) mla_fold_kernel(const MlaPrepParams p)
{
    const int b = blockIdx.x, tid = threadIdx.x;        // thread = channel
    const float a = mla_fold_channel<DT>(p, b, tid);
    if (tid < MLA_DV) {
        p.v_scale[(long)b * MLA_DV + tid] = a / 448.0f;
        p.ws[(long)b * mla_ws_per_sample(p.nchunk) + (long)p.nchunk * MLA_WS_PER_CHUNK + tid] = a;
    }
}

template <int DT>
__global__ void __launch_bounds__(256) mla_quant_kernel(const MlaPrepParams p)
{
    __shared__ MlaTileLds s;
    const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int kvlen = mla_kv_len(p.kv_lens, b, p.Lk);
    if (tile * BLKK >= kvlen) return;                   // (workgroup-uniform) the attention kernel reads the tiles in front of the length only
    const uint16_t *base = reinterpret_cast<const uint16_t *>(p.kv) + (long)b * p.kv_sb + (long)tile * BLKK * p.kv_sl;
    const long kv_sl = p.kv_sl;
    auto row_of = [=](int r) { return base + (long)r * kv_sl; };
    const long bt = (long)b * p.ntile + tile;
    mla_tile_constants<DT>(s, reinterpret_cast<const uint16_t *>(p.k_mean) + (long)b * MLA_DQK,
                           p.ws + (long)b * mla_ws_per_sample(p.nchunk) + (long)p.nchunk * MLA_WS_PER_CHUNK, tid);
    __syncthreads();
    mla_quant_k_tile<DT>(s, row_of, kvlen - tile * BLKK, p.smooth_k != 0, p.k_img + bt * MLA_K_TILE_BYTES, p.k_scale + bt * 4, tid);
    mla_quant_v_tile<DT, false>(s, row_of, kvlen - tile * BLKK, p.v_img + bt * MLA_V_TILE_BYTES, tid);
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
