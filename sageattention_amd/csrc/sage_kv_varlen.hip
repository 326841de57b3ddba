// sage_kv_varlen.hip -- the paged cache's append of PACKED new rows (include/sage_kvpvarlen_gfx950.h): sage_kv_paged.hip's append
// with sample b's rows taken from row cu_seqlens[b] of k_new / v_new [total, Hkv, D] instead of slab b of [B, Hkv, T, D].  Same arithmetic
// through sage_kv_block.h and the same body (sage_kv_append_body.h); the commit launch is a twin of sage_kv_cache.hip's with the same one change.
// A unit of its own: kernels added to sage_kv_cache.hip renumber the registers of the kernels already there.
//
// Replaces in the reference: nothing (no KV cache there).
//
// Ordering and ownership are sage_kv_cache.hip's: launch 1 reads lens and the tails and writes the pool, workgroup (j, h, b) owning logical block
// lens[b] / 64 + j; launch 2 writes the tails and lens, workgroup b alone touching sample b's.  No atomics, no host read.
#include "../../include/sage_gfx950.h"
#include "../../include/sage_kvpvarlen_gfx950.h"
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_quant_math.h"
#include "sage_kv_block.h"
#include "sage_kv_cache.h"
#include "sage_ragged.h"

namespace sage {

// append_range (sage_kv_cache.h) for packed rows: the rows sample b holds, the rows this call gives it -- its stretch of the prefix array,
// clamped by ragged_rows to the packed tensor and to p.T = max_new, then to what still fits -- and the first of them
__device__ __forceinline__ void ragged_append_range(const KvCacheParams &p, const RaggedArgs &r, int b, int &len0, int &t, int &new0)
{
    const int l = p.lens[b];
    len0 = l < 0 ? 0 : (l > p.cap ? p.cap : l);
    int n;
    ragged_rows(r.cu_q[b], r.cu_q[b + 1], r.total_q, p.T, new0, n);
    t = n < p.cap - len0 ? n : p.cap - len0;
}

template <int D, int DT>
__global__ void __launch_bounds__(256)
kvpvarlen_append_kernel(const KvCacheParams p, const PagedArgs g, const RaggedArgs r)
{
#define SAGE_KV_APPEND_PAGED 1
#define SAGE_KV_APPEND_RAGGED 1
#include "sage_kv_append_body.h"
#undef SAGE_KV_APPEND_RAGGED
#undef SAGE_KV_APPEND_PAGED
}

// launch 2, kvcache_commit_kernel's twin: the raw rows of the block the NEXT append opens, from the sample's packed rows, then the new length
__global__ void __launch_bounds__(256)
kvpvarlen_commit_kernel(const KvCacheParams p, const RaggedArgs r)
{
    const int tid = threadIdx.x, b = blockIdx.x;
    int len0, t, new0;
    ragged_append_range(p, r, b, len0, t, new0);
    const int len1 = len0 + t;
    const int open0 = len1 / BLKK * BLKK;           // first row of the open block (== len1: it holds no row yet)
    const int lo = len0 > open0 ? len0 : open0;     // its rows lo .. len1 - 1 are new; those in front of lo (same block as before) are in the tails
    const int n = len1 - lo;                        // 0 .. 63
    const int tpr = p.D / 8;
    for (int h = 0; h < p.H; h++) {
        const long bh = (long)b * p.H + h;
        const uint16_t *k_new = p.k_new + (long)h * p.k_sh + ((long)new0 + (lo - len0)) * p.k_sl;
        const uint16_t *v_new = p.v_new + (long)h * p.v_sh + ((long)new0 + (lo - len0)) * p.v_sl;
        uint16_t *k_tail = p.k_tail + (bh * BLKK + (lo - open0)) * p.D;
        uint16_t *v_tail = p.v_tail + (bh * BLKK + (lo - open0)) * p.D;
        for (int piece = tid; piece < n * tpr; piece += 256) {
            const int rr = piece / tpr, c8 = (piece % tpr) * 8;
            *reinterpret_cast<v4u *>(k_tail + rr * p.D + c8) = *reinterpret_cast<const v4u *>(k_new + (long)rr * p.k_sl + c8);
            *reinterpret_cast<v4u *>(v_tail + rr * p.D + c8) = *reinterpret_cast<const v4u *>(v_new + (long)rr * p.v_sl + c8);
        }
    }
    __syncthreads();                                // every thread has read lens[b]
    if (tid == 0) p.lens[b] = len1;
}

static hipError_t launch_kvpvarlen_append(const KvCacheParams &p, const PagedArgs &g, const RaggedArgs &r, int dtype, hipStream_t s)
{
    const dim3 grid((63 + p.T + BLKK - 1) / BLKK, p.H, p.B);
#define SAGE_KVV(D_, T_) hipLaunchKernelGGL((kvpvarlen_append_kernel<D_, T_>), grid, dim3(256), 0, s, p, g, r)
    if (p.D == 128) { if (dtype == DT_F16) SAGE_KVV(128, DT_F16); else SAGE_KVV(128, DT_BF16); }
    else if (p.D == 64) { if (dtype == DT_F16) SAGE_KVV(64, DT_F16); else SAGE_KVV(64, DT_BF16); }
    else return hipErrorInvalidValue;
#undef SAGE_KVV
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(kvpvarlen_commit_kernel, dim3(p.B), dim3(256), 0, s, p, r);
    return hipGetLastError();
}

}  // namespace sage

extern "C" {

SAGE_KVPVARLEN_API int sage_kvpvarlen_abi_version(void) { return SAGE_KVPVARLEN_ABI_VERSION; }

SAGE_KVPVARLEN_API int sage_kvpvarlen_append(int8_t *k_int8, float *k_scale, void *v_image, float *v_scale, const float *v_amax, const void *k_mean,
                                             void *k_tail, void *v_tail, int32_t *lens,
                                             const void *k_new, const void *v_new, const int32_t *cu_seqlens,
                                             int B, int Hkv, int total, int max_new, int head_dim,
                                             int64_t k_sl, int64_t k_sh, int64_t v_sl, int64_t v_sh,
                                             int dtype,
                                             const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                             void *stream)
{
    const char *const e = "sage_kvpvarlen_append";
    // (T = max_new: the grid's size and the most rows a sample takes; no new_lens, no batch stride)
    sage::KvCacheParams p = sage::kv_append_params(k_int8, k_scale, v_image, v_scale, v_amax, k_mean, k_tail, v_tail, lens, k_new, v_new, nullptr,
                                                   B, Hkv, 0, max_new, head_dim, 0, k_sh, k_sl, 0, v_sh, v_sl);
    sage::PagedArgs g;
    if (const int rc = sage::kv_check_pointers(e, p)) return rc;
    SAGE_REQUIRE(cu_seqlens, "%s: null cu_seqlens", e);
    if (const int rc = sage::paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    p.cap = max_pages_per_seq * page_size;          // (the logical capacity: at most 2^30, checked above)
    if (const int rc = sage::kv_check_batch(e, B, Hkv)) return rc;
    if (const int rc = sage::kv_check_rows(e, p)) return rc;
    SAGE_REQUIRE(total >= 1, "%s: total must be at least 1 (got %d)", e, total);
    if (const int rc = sage::kv_check_dtype_aligned(e, p, dtype)) return rc;
    if (const int rc = sage::paged_check_table_aligned(e, block_table)) return rc;
    SAGE_REQUIRE((reinterpret_cast<uintptr_t>(cu_seqlens) & 3u) == 0, "%s: cu_seqlens must be 4-byte aligned", e);
    if (const int rc = sage::kv_check_strides(e, p)) return rc;
    const sage::RaggedArgs r{cu_seqlens, total};
    const hipError_t err = sage::launch_kvpvarlen_append(p, g, r, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return sage::set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
