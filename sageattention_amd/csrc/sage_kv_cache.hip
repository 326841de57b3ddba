// sage_kv_cache.hip -- the appendable quantised KV cache (include/sage_kvcache_gfx950.h): rows appended in place to the operands of
// sage_attn_fused_q_pv_f8_kvlens, with the K mean and the V abs-max frozen at seeding time.
//
// Replaces in the reference: nothing (no KV cache there; core.py:636-826 quantises the whole K / V per call).
//
// With frozen statistics a row's INT8 bytes depend on its 64-key block alone (per-thread groups are local to a block, sage_quant_math.h
// group_of_row) and its e4m3 byte on the row alone, so an append re-forms the blocks that receive a row and nothing else.  Only the OPEN block
// -- the one a sample's next row goes to -- holds rows from an earlier append; its group abs-maxima run over valid rows only and change as it
// grows, so its raw rows are kept (k_tail / v_tail) and it is re-quantised from them each time.  The arithmetic is the pre-pass's own
// (sage_kv_block.h): quant_int8_kernel's for GR_THREAD_K / QS_TRITON_THREAD, prep_v_kernel<.., FP8>'s with am = v_amax.
//
// Ordering.  Launch 1 (append) reads lens and the tails and writes k_int8 / k_scale / v_image / v_scale; workgroup (j, h, b) owns block
// lens[b] / 64 + j of head h, so no two workgroups write the same byte.  Launch 2 (commit) writes the tails and lens; workgroup b alone touches
// sample b's, every thread of it has read lens[b] before the barrier in front of the one store to it, and stream order puts the launch behind
// every read of launch 1 and in front of the next call's.  No atomics, no host read: the grids follow from the shapes.
#include "../../include/sage_gfx950.h"
#include "../../include/sage_kvcache_gfx950.h"
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_quant_math.h"
#include "sage_kv_block.h"

namespace sage {

struct KvCacheParams {
    int8_t *k_int8;             // [B,H,cap,D]
    float *k_scale;             // [B,H,cap/64*4]
    unsigned char *v_image;     // [B,H,cap/64,D,64]
    float *v_scale;             // [B,H,D]
    const float *v_amax;        // [B,H,D]
    const uint16_t *k_mean;     // nullable [B,H,D]
    uint16_t *k_tail, *v_tail;  // [B,H,64,D]
    int32_t *lens;              // [B]
    const uint16_t *k_new, *v_new;   // [B,H,T,D], strides below
    const int32_t *new_lens;    // nullable [B]
    int B, H, cap, T, D;
    long k_sb, k_sh, k_sl;
    long v_sb, v_sh, v_sl;
    float scale_max;            // 448 (e4m3)
};

// rows sample b holds (clamped to [0, cap]) and rows this call gives it: clamped to [0, T], then to what still fits
__device__ __forceinline__ void append_range(const KvCacheParams &p, int b, int &len0, int &t)
{
    const int l = p.lens[b];
    len0 = l < 0 ? 0 : (l > p.cap ? p.cap : l);
    int n = p.new_lens != nullptr ? p.new_lens[b] : p.T;
    n = n < 0 ? 0 : (n > p.T ? p.T : n);
    t = n < p.cap - len0 ? n : p.cap - len0;
}

template <int D, int DT>
__global__ void __launch_bounds__(256)
kvcache_append_kernel(const KvCacheParams p)
{
    constexpr int CPR = D / 16;                 // 16-element chunks per row
    constexpr int NCH = BLKK * CPR / 256;       // chunks per thread
    constexpr int LDT = D + 8;                  // padded row (16-B aligned), as prep_v_kernel
    __shared__ unsigned gmax[4];
    __shared__ __attribute__((aligned(16))) uint16_t tile[BLKK * LDT];

    const int tid = threadIdx.x;
    const int j = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const long bh = (long)b * p.H + h;
    int len0, t;
    append_range(p, b, len0, t);
    // the scales of the frozen abs-max (every call: the same bytes; a sample that never gets a row has them too)
    if (j == 0 && tid < D) p.v_scale[bh * D + tid] = fp8_v_scale(p.v_amax[bh * D + tid], p.scale_max);
    const int len1 = len0 + t;                  // <= cap
    const int blk = len0 / BLKK + j;
    const int row0 = blk * BLKK;
    if (row0 >= len1) return;                   // no new row for this block (t == 0 included); row0 < len1 <= cap: the block exists
    const int valid = len1 - row0 < BLKK ? len1 - row0 : BLKK;
    const int old = len0 - row0;                // rows r < old of the block are the tails' (j = 0), the rest k_new's / v_new's
    const uint16_t *k_new = p.k_new + (long)b * p.k_sb + (long)h * p.k_sh + (long)(row0 - len0) * p.k_sl;     // row r of the block
    const uint16_t *v_new = p.v_new + (long)b * p.v_sb + (long)h * p.v_sh + (long)(row0 - len0) * p.v_sl;
    const uint16_t *k_tail = p.k_tail + bh * (BLKK * D);
    const uint16_t *v_tail = p.v_tail + bh * (BLKK * D);

    if (tid < 4) gmax[tid] = 0u;
    // V rows -> LDS, zero behind the last valid token
    constexpr int TPR = D / 8;
#pragma unroll
    for (int i = 0; i < BLKK * TPR / 256; i++) {
        const int piece = tid + 256 * i;
        const int r = piece / TPR, c8 = (piece % TPR) * 8;
        v4u raw = {0u, 0u, 0u, 0u};
        if (r < valid) raw = *reinterpret_cast<const v4u *>(r < old ? v_tail + r * D + c8 : v_new + (long)r * p.v_sl + c8);
        *reinterpret_cast<v4u *>(&tile[r * LDT + c8]) = raw;
    }
    __syncthreads();

    // ---- INT8 K: quant_int8_kernel for GR_THREAD_K / QS_TRITON_THREAD over the block's valid rows
    const uint16_t *mean = p.k_mean != nullptr ? p.k_mean + bh * D : nullptr;
    float v[NCH][16];
#pragma unroll
    for (int i = 0; i < NCH; i++) {
        const int c = tid + 256 * i;
        const int r = c / CPR, col = (c % CPR) * 16;
        if (r < valid) {
            const v4u *src = reinterpret_cast<const v4u *>(r < old ? k_tail + r * D + col : k_new + (long)r * p.k_sl + col);
            v4u raw[2] = {src[0], src[1]};
            v4u mraw[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
            if (mean != nullptr) {
                const v4u *ms = reinterpret_cast<const v4u *>(mean + col);
                mraw[0] = ms[0];
                mraw[1] = ms[1];
            }
            const float amax = quant_load16<DT>(raw, mraw, mean != nullptr, QS_TRITON_THREAD, 1.0f, v[i]);
            atomicMax(&gmax[group_of_row(r, GR_THREAD_K, BLKK)], __float_as_uint(amax));
        } else {
#pragma unroll
            for (int e = 0; e < 16; e++) v[i][e] = 0.0f;
        }
    }
    __syncthreads();

    if (tid < 4) p.k_scale[bh * (p.cap / BLKK * 4) + blk * 4 + tid] = quant_scale(__uint_as_float(gmax[tid]), QS_TRITON_THREAD);
    int8_t *k_out = p.k_int8 + (bh * p.cap + row0) * D;
#pragma unroll
    for (int i = 0; i < NCH; i++) {
        const int c = tid + 256 * i;
        const int r = c / CPR, col = (c % CPR) * 16;
        if (r >= valid) continue;
        const float am = __uint_as_float(gmax[group_of_row(r, GR_THREAD_K, BLKK)]);
        const v4u pk = quant_pack16(v[i], am, QS_TRITON_THREAD);
        *reinterpret_cast<v4u *>(k_out + r * D + col) = pk;        // (the attention call that follows reads it: no non-temporal hint)
    }

    // ---- FP8 V: the block's whole tile image, prep_v_kernel<.., FP8> with am = v_amax
    const float *amx = p.v_amax + bh * D;
    unsigned char *out = p.v_image + (bh * (p.cap / BLKK) + blk) * (long)(D * 64);
#pragma unroll
    for (int i = 0; i < D * 4 / 256; i++) {
        const int piece = tid + 256 * i;
        const int d = piece >> 2, pc = piece & 3;
        const v4u pk = fp8_v_image_piece<DT, LDT>(tile, d, pc, 0.0f, fp8_v_recp(amx[d], p.scale_max), false, valid);
        *reinterpret_cast<v4u *>(out + d * 64 + pc * 16) = pk;
    }
}

// launch 2: the raw rows of the block the NEXT append opens, then the new length
__global__ void __launch_bounds__(256)
kvcache_commit_kernel(const KvCacheParams p)
{
    const int tid = threadIdx.x, b = blockIdx.x;
    int len0, t;
    append_range(p, b, len0, t);
    const int len1 = len0 + t;
    const int open0 = len1 / BLKK * BLKK;           // first row of the open block (== len1: it holds no row yet)
    const int lo = len0 > open0 ? len0 : open0;     // its rows lo .. len1 - 1 are new; those in front of lo (same block as before) are in the tails
    const int n = len1 - lo;                        // 0 .. 63
    const int tpr = p.D / 8;
    for (int h = 0; h < p.H; h++) {
        const long bh = (long)b * p.H + h;
        const uint16_t *k_new = p.k_new + (long)b * p.k_sb + (long)h * p.k_sh + (long)(lo - len0) * p.k_sl;
        const uint16_t *v_new = p.v_new + (long)b * p.v_sb + (long)h * p.v_sh + (long)(lo - len0) * p.v_sl;
        uint16_t *k_tail = p.k_tail + (bh * BLKK + (lo - open0)) * p.D;
        uint16_t *v_tail = p.v_tail + (bh * BLKK + (lo - open0)) * p.D;
        for (int piece = tid; piece < n * tpr; piece += 256) {
            const int r = piece / tpr, c8 = (piece % tpr) * 8;
            *reinterpret_cast<v4u *>(k_tail + r * p.D + c8) = *reinterpret_cast<const v4u *>(k_new + (long)r * p.k_sl + c8);
            *reinterpret_cast<v4u *>(v_tail + r * p.D + c8) = *reinterpret_cast<const v4u *>(v_new + (long)r * p.v_sl + c8);
        }
    }
    __syncthreads();                                // every thread has read lens[b]
    if (tid == 0) p.lens[b] = len1;
}

static hipError_t launch_kvcache_append(const KvCacheParams &p, int dtype, hipStream_t s)
{
    const dim3 grid((63 + p.T + BLKK - 1) / BLKK, p.H, p.B);
#define SAGE_KVC(D_, T_) hipLaunchKernelGGL((kvcache_append_kernel<D_, T_>), grid, dim3(256), 0, s, p)
    if (p.D == 128) { if (dtype == DT_F16) SAGE_KVC(128, DT_F16); else SAGE_KVC(128, DT_BF16); }
    else if (p.D == 64) { if (dtype == DT_F16) SAGE_KVC(64, DT_F16); else SAGE_KVC(64, DT_BF16); }
    else return hipErrorInvalidValue;
#undef SAGE_KVC
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(kvcache_commit_kernel, dim3(p.B), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace sage

#define KVC_REQUIRE(cond, ...) do { if (!(cond)) return sage::set_last_error(SAGE_EINVAL, __VA_ARGS__); } while (0)

extern "C" {

SAGE_KVCACHE_API int sage_kvcache_abi_version(void) { return SAGE_KVCACHE_ABI_VERSION; }

SAGE_KVCACHE_API int sage_kvcache_append(int8_t *k_int8, float *k_scale, void *v_image, float *v_scale, const float *v_amax, const void *k_mean,
                                         void *k_tail, void *v_tail, int32_t *lens,
                                         const void *k_new, const void *v_new, const int32_t *new_lens,
                                         int B, int Hkv, int capacity, int T, int head_dim,
                                         int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                         int64_t v_sb, int64_t v_sh, int64_t v_sl,
                                         int dtype, void *stream)
{
    auto a16 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
    KVC_REQUIRE(k_int8 && k_scale && v_image && v_scale && v_amax && k_tail && v_tail && lens,
                "sage_kvcache_append: null cache pointer (only k_mean may be null)");
    KVC_REQUIRE(k_new && v_new, "sage_kvcache_append: null k_new / v_new pointer");
    KVC_REQUIRE(head_dim == 64 || head_dim == 128, "sage_kvcache_append: head_dim must be 64 or 128 (got %d)", head_dim);
    KVC_REQUIRE(T >= 1, "sage_kvcache_append: T must be at least 1 (got %d)", T);
    KVC_REQUIRE(capacity > 0 && capacity % 64 == 0, "sage_kvcache_append: capacity must be a positive multiple of 64 (got %d)", capacity);
    KVC_REQUIRE(B > 0 && B <= 65535 && Hkv > 0 && Hkv <= 65535, "sage_kvcache_append: B and Hkv must be in [1, 65535] (got %d, %d)", B, Hkv);
    KVC_REQUIRE(dtype == SAGE_DTYPE_F16 || dtype == SAGE_DTYPE_BF16, "sage_kvcache_append: bad dtype %d", dtype);
    KVC_REQUIRE(a16(k_int8) && a16(k_scale) && a16(v_image) && a16(k_tail) && a16(v_tail) && a16(k_new) && a16(v_new) && (!k_mean || a16(k_mean)),
                "sage_kvcache_append: k_int8 / k_scale / v_image / k_mean / k_tail / v_tail / k_new / v_new must be 16-byte aligned");
    KVC_REQUIRE(k_sb % 8 == 0 && k_sh % 8 == 0 && k_sl % 8 == 0 && v_sb % 8 == 0 && v_sh % 8 == 0 && v_sl % 8 == 0,
                "sage_kvcache_append: k_new / v_new strides must be multiples of 8 elements");
    sage::KvCacheParams p{};
    p.k_int8 = k_int8; p.k_scale = k_scale; p.v_image = static_cast<unsigned char *>(v_image); p.v_scale = v_scale; p.v_amax = v_amax;
    p.k_mean = static_cast<const uint16_t *>(k_mean);
    p.k_tail = static_cast<uint16_t *>(k_tail); p.v_tail = static_cast<uint16_t *>(v_tail); p.lens = lens;
    p.k_new = static_cast<const uint16_t *>(k_new); p.v_new = static_cast<const uint16_t *>(v_new); p.new_lens = new_lens;
    p.B = B; p.H = Hkv; p.cap = capacity; p.T = T; p.D = head_dim;
    p.k_sb = k_sb; p.k_sh = k_sh; p.k_sl = k_sl; p.v_sb = v_sb; p.v_sh = v_sh; p.v_sl = v_sl;
    p.scale_max = 448.0f;
    const hipError_t e = sage::launch_kvcache_append(p, dtype, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return sage::set_last_error(SAGE_ELAUNCH, "sage_kvcache_append launch: %s", hipGetErrorString(e));
    return SAGE_OK;
}

}  // extern "C"
