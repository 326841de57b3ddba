// sage_qk192_prepass.hip -- the K / V pre-pass of the 192-wide Q / K, 128-wide V route (include/sage_qk192_gfx950.h), gfx950.
//
// Two launches, as the head_dim = 256 route's and for its reason: the K mean and the V amax are statistics over ALL tokens of a (batch, kv
// head) and every tile's bytes depend on them.
//   1. qk192_stats_kernel   one workgroup per 256-token chunk: per-channel K sum (192) and V amax (128) of the chunk into the workspace, 320
//                           floats per chunk (no atomics: the result does not depend on the order of execution).
//   2. qk192_quant_kernel   one workgroup per 64-key tile: folds the chunks' statistics in ascending order (L2 hits: 1.25 KiB per chunk),
//                           then quantises its 64 K rows into the three panels of the K image and its 64 V rows into the V image.
// Thread mappings: K rows are 24 columns of 8 channels (16-byte loads) and V rows 16, so the statistics kernel runs 8 row groups x 24 columns
// on threads 0 .. 191 for K and 16 row groups x 16 columns on all 256 for V; the quantiser gives a K row to four threads of 48 channels
// (three 16-byte chunks of the image each) and deals the 64 x 16 V columns of a tile four to a thread.
// HBM traffic per element: K and V are read twice (2 + 2 bytes) and written once as one byte -- 5 bytes per element of each.
#include "../../include/sage_qk192_gfx950.h"
#include "sage_qk192.h"
#include "sage_qk192_prep.h"
#include "sage_host_checks.h"

namespace sage {

// The work of a chunk and of a tile is sage_qk192_prep.h's, shared with the packed pre-pass; these kernels say which chunk and which tile.
template <int DT>
__global__ void __launch_bounds__(256) qk192_stats_kernel(const Qk192PrepParams p)
{
    const int chunk = blockIdx.x, bh = blockIdx.y, b = bh / p.Hkv, hk = bh % p.Hkv;
    qk192_stats_chunk<DT>(reinterpret_cast<const uint16_t *>(p.k) + (long)b * p.k_sb + (long)hk * p.k_sh,
                          reinterpret_cast<const uint16_t *>(p.v) + (long)b * p.v_sb + (long)hk * p.v_sh, p.k_sl, p.v_sl, chunk, p.Lk,
                          p.ws + ((long)bh * p.nchunk + chunk) * QK192_WS_PER_CHUNK);
}

template <int DT>
__global__ void __launch_bounds__(256) qk192_quant_kernel(const Qk192PrepParams p)
{
    const int tile = blockIdx.x, bh = blockIdx.y, b = bh / p.Hkv, hk = bh % p.Hkv;
    Qk192TileOut out;
    out.k_mean = reinterpret_cast<uint16_t *>(p.k_mean) + (long)bh * QK192_DQK;
    out.v_scale = p.v_scale + (long)bh * QK192_DV;
    out.k_scale = p.k_scale + ((long)bh * p.ntile + tile) * 4;
    out.k_img = p.k_img + ((long)bh * p.ntile + tile) * QK192_K_TILE_BYTES;
    out.v_img = p.v_img + ((long)bh * p.ntile + tile) * QK192_V_TILE_BYTES;
    qk192_quant_tile<DT>(reinterpret_cast<const uint16_t *>(p.k) + (long)b * p.k_sb + (long)hk * p.k_sh,
                         reinterpret_cast<const uint16_t *>(p.v) + (long)b * p.v_sb + (long)hk * p.v_sh, p.k_sl, p.v_sl, tile, p.Lk,
                         p.ws + (long)bh * p.nchunk * QK192_WS_PER_CHUNK, p.nchunk, p.smooth_k != 0, out);
}

hipError_t launch_qk192_prepass(const Qk192PrepParams &p, int dtype, hipStream_t stream)
{
    const dim3 g1(p.nchunk, p.B * p.Hkv), g2(p.ntile, p.B * p.Hkv);
    if (dtype == DT_F16) {
        hipLaunchKernelGGL(qk192_stats_kernel<DT_F16>, g1, dim3(256), 0, stream, p);
        hipLaunchKernelGGL(qk192_quant_kernel<DT_F16>, g2, dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(qk192_stats_kernel<DT_BF16>, g1, dim3(256), 0, stream, p);
        hipLaunchKernelGGL(qk192_quant_kernel<DT_BF16>, g2, dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

// a tensor of [B, H, L, width] halves behind element strides: 16-byte rows
static bool qk192_tensor_ok(const void *ptr, int64_t sb, int64_t sh, int64_t sl, int width)
{
    return aligned16_strides(ptr, 8, sb, sh, sl) && sb >= 0 && sh >= 0 && sl >= width;
}

}  // namespace sage

extern "C" {

using namespace sage;

SAGE_QK192_API int64_t sage_qk192_ws_floats(int B, int Hkv, int Lk)
{
    if (B < 1 || Hkv < 1 || Lk < 1) return set_last_error(SAGE_EINVAL, "sage_qk192_ws_floats: empty problem (B %d, Hkv %d, Lk %d)", B, Hkv, Lk);
    return (int64_t)B * Hkv * ((Lk + QK192_CHUNK - 1) / QK192_CHUNK) * QK192_WS_PER_CHUNK;
}

SAGE_QK192_API int sage_qk192_prepass(const void *k, const void *v, void *k_image, float *k_scale, void *k_mean, void *v_image, float *v_scale,
                                      float *ws, int64_t ws_floats, int B, int Hkv, int Lk, int head_dim_qk, int head_dim_v,
                                      int64_t k_sb, int64_t k_sh, int64_t k_sl, int64_t v_sb, int64_t v_sh, int64_t v_sl,
                                      int smooth_k, int dtype, void *stream)
{
    const char *const e = "sage_qk192_prepass";
    SAGE_REQUIRE(head_dim_qk == QK192_DQK && head_dim_v == QK192_DV,
                 "%s: head_dim_qk must be 192 and head_dim_v 128 (got %d and %d); zero-pad 129 .. 191 / 1 .. 127, and call sage_hd256_prepass for wider rows, sage_prepass_kv for 64 / 128",
                 e, head_dim_qk, head_dim_v);
    SAGE_REQUIRE(dtype == DT_F16 || dtype == DT_BF16, "%s: dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got %d)", e, dtype);
    SAGE_REQUIRE(B >= 1 && Hkv >= 1 && Lk >= 1, "%s: empty problem (B %d, Hkv %d, Lk %d)", e, B, Hkv, Lk);
    SAGE_REQUIRE(k && v && k_image && k_scale && k_mean && v_image && v_scale && ws, "%s: null pointer", e);
    SAGE_REQUIRE(qk192_tensor_ok(k, k_sb, k_sh, k_sl, QK192_DQK) && qk192_tensor_ok(v, v_sb, v_sh, v_sl, QK192_DV),
                 "%s: k and v must be 16-byte aligned with non-negative strides in multiples of 8 elements and a token stride of at least 192 (k) / 128 (v)", e);
    SAGE_REQUIRE(aligned16(k_image) && aligned16(v_image) && aligned4(k_scale) && aligned4(v_scale) && aligned4(ws) && (reinterpret_cast<uintptr_t>(k_mean) & 1u) == 0,
                 "%s: the images must be 16-byte aligned, k_scale, v_scale and ws 4-byte, k_mean 2-byte", e);
    const int64_t need = sage_qk192_ws_floats(B, Hkv, Lk);
    SAGE_REQUIRE(ws_floats >= need, "%s: ws holds %lld floats, sage_qk192_ws_floats(B, Hkv, Lk) = %lld", e, (long long)ws_floats, (long long)need);
    SAGE_REQUIRE((int64_t)B * Hkv <= 65535, "%s: B * Hkv must be at most 65535 (got %lld)", e, (long long)B * Hkv);
    Qk192PrepParams p{};
    p.k = k; p.v = v;
    p.k_img = static_cast<unsigned char *>(k_image); p.v_img = static_cast<unsigned char *>(v_image);
    p.k_scale = k_scale; p.v_scale = v_scale; p.ws = ws; p.k_mean = k_mean;
    p.k_sb = k_sb; p.k_sh = k_sh; p.k_sl = k_sl; p.v_sb = v_sb; p.v_sh = v_sh; p.v_sl = v_sl;
    p.B = B; p.Hkv = Hkv; p.Lk = Lk; p.ntile = (Lk + BLKK - 1) / BLKK; p.nchunk = (Lk + QK192_CHUNK - 1) / QK192_CHUNK; p.smooth_k = smooth_k != 0;
    const hipError_t err = launch_qk192_prepass(p, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
