// sage_hd256_prepass.hip -- the K / V pre-pass of the head_dim = 256 route (include/sage_hd256_gfx950.h), gfx950.
//
// Two launches.  The K mean and the V amax are statistics over ALL tokens of a (batch, kv head) and every tile's bytes depend on them, so one
// launch would need a device-wide barrier (the family's one-launch pre-pass has one and keeps a 512-token slab in registers across it: at
// D = 256 that slab is 256 VGPRs per thread).  Here:
//   1. hd256_stats_kernel   one workgroup per 256-token chunk: per-channel K sum and V amax of the chunk into the workspace (no atomics: the
//                           result does not depend on the order of execution).
//   2. hd256_quant_kernel   one workgroup per 64-key tile: folds the chunks' statistics in ascending order (L2 hits: 2 KiB per chunk), then
//                           quantises its 64 K rows into the K image and its 64 V rows into the V image.
// HBM traffic per element: K and V are read twice (2 + 2 bytes) and written once as one byte -- 5 bytes per element of each.
#include "../../include/sage_hd256_gfx950.h"
#include "sage_hd256.h"
#include "sage_host_checks.h"
#include "sage_quant_math.h"

namespace sage {

// eight consecutive channels of one row: a 16-byte load, zeros for a row past the last token
template <int DT>
__device__ __forceinline__ void hd256_load8(const uint16_t *row, bool ok, float (&x)[8])
{
    v4u raw = {0u, 0u, 0u, 0u};
    if (ok) raw = *reinterpret_cast<const v4u *>(row);
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = ld16<DT>((uint16_t)((j & 1) ? (raw[j >> 1] >> 16) : (raw[j >> 1] & 0xffffu)));
}

// thread = (row group rg of 8, 8-channel column cl of 32): rows rg, rg + 8, .. of the chunk; the eight row groups meet in LDS
template <int DT>
__global__ void __launch_bounds__(256) hd256_stats_kernel(const Hd256PrepParams p)
{
    __shared__ float red[2][8][HD256];
    const int tid = threadIdx.x, cl = tid & 31, rg = tid >> 5;
    const int chunk = blockIdx.x, bh = blockIdx.y, b = bh / p.Hkv, hk = bh % p.Hkv;
    const uint16_t *kb = reinterpret_cast<const uint16_t *>(p.k) + (long)b * p.k_sb + (long)hk * p.k_sh + 8 * cl;
    const uint16_t *vb = reinterpret_cast<const uint16_t *>(p.v) + (long)b * p.v_sb + (long)hk * p.v_sh + 8 * cl;
    float ksum[8], vam[8];
#pragma unroll
    for (int j = 0; j < 8; j++) ksum[j] = vam[j] = 0.0f;
    for (int i = 0; i < HD256_CHUNK / 8; i++) {
        const int tok = chunk * HD256_CHUNK + 8 * i + rg;
        const bool ok = tok < p.Lk;
        float kx[8], vx[8];
        hd256_load8<DT>(kb + (long)tok * p.k_sl, ok, kx);
        hd256_load8<DT>(vb + (long)tok * p.v_sl, ok, vx);
#pragma unroll
        for (int j = 0; j < 8; j++) { ksum[j] += kx[j]; vam[j] = fmaxf(vam[j], fabsf(vx[j])); }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) { red[0][rg][8 * cl + j] = ksum[j]; red[1][rg][8 * cl + j] = vam[j]; }
    __syncthreads();
    float s = 0.0f, a = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; r++) { s += red[0][r][tid]; a = fmaxf(a, red[1][r][tid]); }
    float *w = p.ws + ((long)bh * p.nchunk + chunk) * (2 * HD256);
    w[tid] = s;
    w[HD256 + tid] = a;
}

template <int DT>
__global__ void __launch_bounds__(256) hd256_quant_kernel(const Hd256PrepParams p)
{
    __shared__ float s_mean[HD256], s_vrecp[HD256], s_ramax[BLKK];
    __shared__ __attribute__((aligned(16))) unsigned char s_img[HD256_TILE_BYTES];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, bh = blockIdx.y, b = bh / p.Hkv, hk = bh % p.Hkv;

    // ---- the statistics of the (batch, kv head): thread = channel, chunks in ascending order ----
    {
        const float *w = p.ws + (long)bh * p.nchunk * (2 * HD256);
        float s = 0.0f, a = 0.0f;
        for (int c = 0; c < p.nchunk; c++) { s += w[(long)c * (2 * HD256) + tid]; a = fmaxf(a, w[(long)c * (2 * HD256) + HD256 + tid]); }
        // the reference's mean is the FP32 sum over Lk, rounded to the input dtype (core.py:773); without smooth_k nothing is subtracted
        const uint16_t m16 = p.smooth_k ? st16<DT>(s / (float)p.Lk) : (uint16_t)0;
        s_mean[tid] = ld16<DT>(m16);
        s_vrecp[tid] = a > 0.0f ? 448.0f / a : 0.0f;          // (a channel of zeros -- head_dim padding -- gives zero bytes, not 0 * inf)
        if (tile == 0) {
            reinterpret_cast<uint16_t *>(p.k_mean)[(long)bh * HD256 + tid] = m16;
            p.v_scale[(long)bh * HD256 + tid] = a / 448.0f;
        }
    }
    __syncthreads();

    // ---- K: thread = (row r of 64, quarter qd of the row's 256 channels) ----
    {
        const int r = tid >> 2, qd = tid & 3;
        const int key = tile * BLKK + r;
        const bool ok = key < p.Lk;
        const uint16_t *row = reinterpret_cast<const uint16_t *>(p.k) + (long)b * p.k_sb + (long)hk * p.k_sh + (long)key * p.k_sl + 64 * qd;
        float x[64];
        float amax = 0.0f;
#pragma unroll
        for (int v = 0; v < 8; v++) {
            float f[8];
            hd256_load8<DT>(row + 8 * v, ok, f);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                // k - mean in the input dtype (core.py:775), as the reference's quantiser receives it
                const float d = p.smooth_k ? ld16<DT>(st16<DT>(f[j] - s_mean[64 * qd + 8 * v + j])) : f[j];
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
        if (tid < 4) p.k_scale[((long)bh * p.ntile + tile) * 4 + tid] = group_scale(tid);
        const float sc = group_scale((r & 7) >> 1);
        const float y = quant_recip(sc);
        unsigned char *out = p.k_img + ((long)bh * p.ntile + tile) * HD256_TILE_BYTES + r * HD256;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            v4u pk;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                int q8[4];
#pragma unroll
                for (int j = 0; j < 4; j++) q8[j] = quant_round_triton_nz(x[16 * c + 4 * w + j], sc, y);
                pk[w] = pack_int8x4(q8[0], q8[1], q8[2], q8[3]);
            }
            *reinterpret_cast<v4u *>(out + hd256_k_chunk(r, 4 * qd + c) * 16) = pk;
        }
    }

    // ---- V: 64 rows of 16-byte loads, e4m3 bytes scattered into the image in LDS, the image copied out linearly ----
    {
        const uint16_t *vb = reinterpret_cast<const uint16_t *>(p.v) + (long)b * p.v_sb + (long)hk * p.v_sh;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int e = tid + 256 * i, t = e >> 5, cv = e & 31;
            const int tok = tile * BLKK + t;
            float f[8];
            hd256_load8<DT>(vb + (long)tok * p.v_sl + 8 * cv, tok < p.Lk, f);
            const int pos = hd256_position_of_token(t);
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const int d = 8 * cv + j;
                const int w = __builtin_amdgcn_cvt_pk_fp8_f32(f[j] * s_vrecp[d], f[j + 1] * s_vrecp[d + 1], 0, false);
                s_img[d * 64 + swz_chunk<64>(d, pos >> 4) * 16 + (pos & 15)] = (unsigned char)(w & 0xff);
                s_img[(d + 1) * 64 + swz_chunk<64>(d + 1, pos >> 4) * 16 + (pos & 15)] = (unsigned char)((w >> 8) & 0xff);
            }
        }
        __syncthreads();
        unsigned char *out = p.v_img + ((long)bh * p.ntile + tile) * HD256_TILE_BYTES;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int e = tid + 256 * i;
            *reinterpret_cast<v4u *>(out + e * 16) = *reinterpret_cast<const v4u *>(s_img + e * 16);
        }
    }
}

hipError_t launch_hd256_prepass(const Hd256PrepParams &p, int dtype, hipStream_t stream)
{
    const dim3 g1(p.nchunk, p.B * p.Hkv), g2(p.ntile, p.B * p.Hkv);
    if (dtype == DT_F16) {
        hipLaunchKernelGGL(hd256_stats_kernel<DT_F16>, g1, dim3(256), 0, stream, p);
        hipLaunchKernelGGL(hd256_quant_kernel<DT_F16>, g2, dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(hd256_stats_kernel<DT_BF16>, g1, dim3(256), 0, stream, p);
        hipLaunchKernelGGL(hd256_quant_kernel<DT_BF16>, g2, dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

// tensors of [B, H, L, 256] halves behind element strides: 16-byte rows, the largest offset inside a long
static bool hd256_tensor_ok(const void *ptr, int64_t sb, int64_t sh, int64_t sl)
{
    return aligned16_strides(ptr, 8, sb, sh, sl) && sb >= 0 && sh >= 0 && sl >= HD256;
}

}  // namespace sage

extern "C" {

using namespace sage;

SAGE_HD256_API int64_t sage_hd256_ws_floats(int B, int Hkv, int Lk)
{
    if (B < 1 || Hkv < 1 || Lk < 1) return set_last_error(SAGE_EINVAL, "sage_hd256_ws_floats: empty problem (B %d, Hkv %d, Lk %d)", B, Hkv, Lk);
    return (int64_t)B * Hkv * ((Lk + HD256_CHUNK - 1) / HD256_CHUNK) * (2 * HD256);
}

SAGE_HD256_API int sage_hd256_prepass(const void *k, const void *v, void *k_image, float *k_scale, void *k_mean, void *v_image, float *v_scale,
                                      float *ws, int64_t ws_floats, int B, int Hkv, int Lk, int head_dim,
                                      int64_t k_sb, int64_t k_sh, int64_t k_sl, int64_t v_sb, int64_t v_sh, int64_t v_sl,
                                      int smooth_k, int dtype, void *stream)
{
    const char *const e = "sage_hd256_prepass";
    SAGE_REQUIRE(head_dim == HD256, "%s: head_dim must be 256 (got %d); zero-pad 129 .. 255 to 256, and call sage_prepass_kv for 64 / 128", e, head_dim);
    SAGE_REQUIRE(dtype == DT_F16 || dtype == DT_BF16, "%s: dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got %d)", e, dtype);
    SAGE_REQUIRE(B >= 1 && Hkv >= 1 && Lk >= 1, "%s: empty problem (B %d, Hkv %d, Lk %d)", e, B, Hkv, Lk);
    SAGE_REQUIRE(k && v && k_image && k_scale && k_mean && v_image && v_scale && ws, "%s: null pointer", e);
    SAGE_REQUIRE(hd256_tensor_ok(k, k_sb, k_sh, k_sl) && hd256_tensor_ok(v, v_sb, v_sh, v_sl),
                 "%s: k and v must be 16-byte aligned with non-negative strides in multiples of 8 elements and a token stride of at least 256", e);
    SAGE_REQUIRE(aligned16(k_image) && aligned16(v_image) && aligned4(k_scale) && aligned4(v_scale) && aligned4(ws) && (reinterpret_cast<uintptr_t>(k_mean) & 1u) == 0,
                 "%s: the images must be 16-byte aligned, k_scale, v_scale and ws 4-byte, k_mean 2-byte", e);
    const int64_t need = sage_hd256_ws_floats(B, Hkv, Lk);
    SAGE_REQUIRE(ws_floats >= need, "%s: ws holds %lld floats, sage_hd256_ws_floats(B, Hkv, Lk) = %lld", e, (long long)ws_floats, (long long)need);
    SAGE_REQUIRE((int64_t)B * Hkv <= 65535, "%s: B * Hkv must be at most 65535 (got %lld)", e, (long long)B * Hkv);
    Hd256PrepParams p{};
    p.k = k; p.v = v;
    p.k_img = static_cast<unsigned char *>(k_image); p.v_img = static_cast<unsigned char *>(v_image);
    p.k_scale = k_scale; p.v_scale = v_scale; p.ws = ws; p.k_mean = k_mean;
    p.k_sb = k_sb; p.k_sh = k_sh; p.k_sl = k_sl; p.v_sb = v_sb; p.v_sh = v_sh; p.v_sl = v_sl;
    p.B = B; p.Hkv = Hkv; p.Lk = Lk; p.ntile = (Lk + BLKK - 1) / BLKK; p.nchunk = (Lk + HD256_CHUNK - 1) / HD256_CHUNK; p.smooth_k = smooth_k != 0;
    const hipError_t err = launch_hd256_prepass(p, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
