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
#include "sage_host_checks.h"
#include "sage_quant_math.h"

namespace sage {

// eight consecutive channels of one row: a 16-byte load, zeros for a row past the last token
template <int DT>
__device__ __forceinline__ void qk192_load8(const uint16_t *row, bool ok, float (&x)[8])
{
    v4u raw = {0u, 0u, 0u, 0u};
    if (ok) raw = *reinterpret_cast<const v4u *>(row);
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = ld16<DT>((uint16_t)((j & 1) ? (raw[j >> 1] >> 16) : (raw[j >> 1] & 0xffffu)));
}

template <int DT>
__global__ void __launch_bounds__(256) qk192_stats_kernel(const Qk192PrepParams p)
{
    __shared__ float red_k[8][QK192_DQK], red_v[16][QK192_DV];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x, bh = blockIdx.y, b = bh / p.Hkv, hk = bh % p.Hkv;
    // ---- K: threads 0 .. 191 = (row group of 8, 8-channel column of 24): rows rg, rg + 8, .. of the chunk ----
    if (tid < 192) {
        const int cl = tid % 24, rg = tid / 24;
        const uint16_t *kb = reinterpret_cast<const uint16_t *>(p.k) + (long)b * p.k_sb + (long)hk * p.k_sh + 8 * cl;
        float ksum[8];
#pragma unroll
        for (int j = 0; j < 8; j++) ksum[j] = 0.0f;
        for (int i = 0; i < QK192_CHUNK / 8; i++) {
            const int tok = chunk * QK192_CHUNK + 8 * i + rg;
            float kx[8];
            qk192_load8<DT>(kb + (long)tok * p.k_sl, tok < p.Lk, kx);
#pragma unroll
            for (int j = 0; j < 8; j++) ksum[j] += kx[j];
        }
#pragma unroll
        for (int j = 0; j < 8; j++) red_k[rg][8 * cl + j] = ksum[j];
    }
    // ---- V: all threads = (row group of 16, 8-channel column of 16): rows rg, rg + 16, .. ----
    {
        const int cl = tid & 15, rg = tid >> 4;
        const uint16_t *vb = reinterpret_cast<const uint16_t *>(p.v) + (long)b * p.v_sb + (long)hk * p.v_sh + 8 * cl;
        float vam[8];
#pragma unroll
        for (int j = 0; j < 8; j++) vam[j] = 0.0f;
        for (int i = 0; i < QK192_CHUNK / 16; i++) {
            const int tok = chunk * QK192_CHUNK + 16 * i + rg;
            float vx[8];
            qk192_load8<DT>(vb + (long)tok * p.v_sl, tok < p.Lk, vx);
#pragma unroll
            for (int j = 0; j < 8; j++) vam[j] = fmaxf(vam[j], fabsf(vx[j]));
        }
#pragma unroll
        for (int j = 0; j < 8; j++) red_v[rg][8 * cl + j] = vam[j];
    }
    __syncthreads();
    // the row groups in ascending order: one fixed order of additions per channel
    float *w = p.ws + ((long)bh * p.nchunk + chunk) * QK192_WS_PER_CHUNK;
    if (tid < QK192_DQK) {
        float s = 0.0f;
#pragma unroll
        for (int r = 0; r < 8; r++) s += red_k[r][tid];
        w[tid] = s;
    } else {                                             // threads 192 .. 255: two V channels each
        for (int d = tid - QK192_DQK; d < QK192_DV; d += 64) {
            float a = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; r++) a = fmaxf(a, red_v[r][d]);
            w[QK192_DQK + d] = a;
        }
    }
}

template <int DT>
__global__ void __launch_bounds__(256) qk192_quant_kernel(const Qk192PrepParams p)
{
    __shared__ float s_mean[QK192_DQK], s_vrecp[QK192_DV], s_ramax[BLKK];
    __shared__ __attribute__((aligned(16))) unsigned char s_img[QK192_V_TILE_BYTES];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, bh = blockIdx.y, b = bh / p.Hkv, hk = bh % p.Hkv;

    // ---- the statistics of the (batch, kv head): thread = channel, chunks in ascending order ----
    {
        const float *w = p.ws + (long)bh * p.nchunk * QK192_WS_PER_CHUNK;
        if (tid < QK192_DQK) {
            float s = 0.0f;
            for (int c = 0; c < p.nchunk; c++) s += w[(long)c * QK192_WS_PER_CHUNK + tid];
            // the reference's mean is the FP32 sum over Lk, rounded to the input dtype (core.py:773); without smooth_k nothing is subtracted
            const uint16_t m16 = p.smooth_k ? st16<DT>(s / (float)p.Lk) : (uint16_t)0;
            s_mean[tid] = ld16<DT>(m16);
            if (tile == 0) reinterpret_cast<uint16_t *>(p.k_mean)[(long)bh * QK192_DQK + tid] = m16;
        } else {
            for (int d = tid - QK192_DQK; d < QK192_DV; d += 64) {
                float a = 0.0f;
                for (int c = 0; c < p.nchunk; c++) a = fmaxf(a, w[(long)c * QK192_WS_PER_CHUNK + QK192_DQK + d]);
                s_vrecp[d] = a > 0.0f ? 448.0f / a : 0.0f;          // (a channel of zeros -- head_dim padding -- gives zero bytes, not 0 * inf)
                if (tile == 0) p.v_scale[(long)bh * QK192_DV + d] = a / 448.0f;
            }
        }
    }
    __syncthreads();

    // ---- K: thread = (row r of 64, quarter qd of the row: channels 48 qd .. 48 qd + 47, the image's chunks 3 qd .. 3 qd + 2) ----
    {
        const int r = tid >> 2, qd = tid & 3;
        const int key = tile * BLKK + r;
        const bool ok = key < p.Lk;
        const uint16_t *row = reinterpret_cast<const uint16_t *>(p.k) + (long)b * p.k_sb + (long)hk * p.k_sh + (long)key * p.k_sl + 48 * qd;
        float x[48];
        float amax = 0.0f;
#pragma unroll
        for (int v = 0; v < 6; v++) {
            float f[8];
            qk192_load8<DT>(row + 8 * v, ok, f);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                // k - mean in the input dtype (core.py:775), as the reference's quantiser receives it
                const float d = p.smooth_k ? ld16<DT>(st16<DT>(f[j] - s_mean[48 * qd + 8 * v + j])) : f[j];
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
        unsigned char *out = p.k_img + ((long)bh * p.ntile + tile) * QK192_K_TILE_BYTES;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v4u pk;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                int q8[4];
#pragma unroll
                for (int j = 0; j < 4; j++) q8[j] = quant_round_triton_nz(x[16 * c + 4 * w + j], sc, y);
                pk[w] = pack_int8x4(q8[0], q8[1], q8[2], q8[3]);
            }
            *reinterpret_cast<v4u *>(out + qk192_k_offset(r, 3 * qd + c)) = pk;
        }
    }

    // ---- V: 64 rows of sixteen 16-byte loads, e4m3 bytes scattered into the image in LDS, the image copied out linearly ----
    {
        const uint16_t *vb = reinterpret_cast<const uint16_t *>(p.v) + (long)b * p.v_sb + (long)hk * p.v_sh;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int e = tid + 256 * i, t = e >> 4, cv = e & 15;
            const int tok = tile * BLKK + t;
            float f[8];
            qk192_load8<DT>(vb + (long)tok * p.v_sl + 8 * cv, tok < p.Lk, f);
            const int pos = qk192_position_of_token(t);
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const int d = 8 * cv + j;
                const int w = __builtin_amdgcn_cvt_pk_fp8_f32(f[j] * s_vrecp[d], f[j + 1] * s_vrecp[d + 1], 0, false);
                s_img[qk192_v_offset(d, pos)] = (unsigned char)(w & 0xff);
                s_img[qk192_v_offset(d + 1, pos)] = (unsigned char)((w >> 8) & 0xff);
            }
        }
        __syncthreads();
        unsigned char *out = p.v_img + ((long)bh * p.ntile + tile) * QK192_V_TILE_BYTES;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int e = tid + 256 * i;
            *reinterpret_cast<v4u *>(out + e * 16) = *reinterpret_cast<const v4u *>(s_img + e * 16);
        }
    }
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
