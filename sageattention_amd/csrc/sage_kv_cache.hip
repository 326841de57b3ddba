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
    const char *const e = "sage_kvcache_append";
    const sage::KvCacheParams p = sage::kv_append_params(k_int8, k_scale, v_image, v_scale, v_amax, k_mean, k_tail, v_tail, lens, k_new, v_new, new_lens,
                                                         B, Hkv, capacity, T, head_dim, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl);
    if (const int rc = sage::kv_check_pointers(e, p)) return rc;
    if (const int rc = sage::kv_check_rows(e, p)) return rc;
    SAGE_REQUIRE(capacity > 0 && capacity % 64 == 0, "%s: capacity must be a positive multiple of 64 (got %d)", e, capacity);
    if (const int rc = sage::kv_check_batch(e, B, Hkv)) return rc;
    if (const int rc = sage::kv_check_dtype_aligned(e, p, dtype)) return rc;
    if (const int rc = sage::kv_check_strides(e, p)) return rc;
    const hipError_t err = sage::launch_kvcache_append(p, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return sage::set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
