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
#include "sage_kv_cache.h"

namespace sage {

template <int D, int DT>
__global__ void __launch_bounds__(256)
kvcache_append_kernel(const KvCacheParams p)
{
#define SAGE_KV_APPEND_PAGED 0
#include "sage_kv_append_body.h"
#undef SAGE_KV_APPEND_PAGED
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

hipError_t launch_kvcache_commit(const KvCacheParams &p, hipStream_t s)
{
    hipLaunchKernelGGL(kvcache_commit_kernel, dim3(p.B), dim3(256), 0, s, p);
    return hipGetLastError();
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
    return launch_kvcache_commit(p, s);
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
