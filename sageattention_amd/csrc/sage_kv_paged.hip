// sage_kv_paged.hip -- the appendable quantised KV cache over a pool of pages (include/sage_kvpaged_gfx950.h): sage_kv_cache.hip's append with
// the block's destination looked up in a block table.  Same arithmetic through sage_kv_block.h and the same body (sage_kv_append_body.h); the
// tails, the lengths and the commit launch are per sequence and are sage_kv_cache.hip's own.
//
// Replaces in the reference: nothing (no KV cache there).
//
// Workgroup (j, h, b) owns logical block lens[b] / 64 + j of head h, as there; two samples share no page (the caller's contract), so no two
// workgroups write the same byte.  A block whose table entry is not a page of the pool is not written.
#include "../../include/sage_gfx950.h"
#include "../../include/sage_kvpaged_gfx950.h"
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_quant_math.h"
#include "sage_kv_block.h"
#include "sage_kv_cache.h"

namespace sage {

// PAGED: k_int8 / k_scale / v_image are a pool of pages of 64 << g.page_shift rows, p.cap the logical capacity g.max_pages pages give a sample;
// the workgroup's logical block lies in page block_table[b][blk >> page_shift]
template <int D, int DT>
__global__ void __launch_bounds__(256)
kvpaged_append_kernel(const KvCacheParams p, const PagedArgs g)
{
#define SAGE_KV_APPEND_PAGED 1
#include "sage_kv_append_body.h"
#undef SAGE_KV_APPEND_PAGED
}

static hipError_t launch_kvpaged_append(const KvCacheParams &p, const PagedArgs &g, int dtype, hipStream_t s)
{
    const dim3 grid((63 + p.T + BLKK - 1) / BLKK, p.H, p.B);
#define SAGE_KVP(D_, T_) hipLaunchKernelGGL((kvpaged_append_kernel<D_, T_>), grid, dim3(256), 0, s, p, g)
    if (p.D == 128) { if (dtype == DT_F16) SAGE_KVP(128, DT_F16); else SAGE_KVP(128, DT_BF16); }
    else if (p.D == 64) { if (dtype == DT_F16) SAGE_KVP(64, DT_F16); else SAGE_KVP(64, DT_BF16); }
    else return hipErrorInvalidValue;
#undef SAGE_KVP
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    return launch_kvcache_commit(p, s);
}

// page_size = 64 * 2^k -> k, or -1
int paged_shift(int page_size)
{
    if (page_size < 64 || (page_size & (page_size - 1)) != 0) return -1;
    int k = 0;
    while ((64 << k) < page_size) k++;
    return k;
}

}  // namespace sage

extern "C" {

SAGE_KVPAGED_API int sage_kvpaged_abi_version(void) { return SAGE_KVPAGED_ABI_VERSION; }

SAGE_KVPAGED_API int sage_kvpaged_append(int8_t *k_int8, float *k_scale, void *v_image, float *v_scale, const float *v_amax, const void *k_mean,
                                         void *k_tail, void *v_tail, int32_t *lens,
                                         const void *k_new, const void *v_new, const int32_t *new_lens,
                                         int B, int Hkv, int T, int head_dim,
                                         int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                         int64_t v_sb, int64_t v_sh, int64_t v_sl,
                                         int dtype,
                                         const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                         void *stream)
{
    const char *const e = "sage_kvpaged_append";
    sage::KvCacheParams p = sage::kv_append_params(k_int8, k_scale, v_image, v_scale, v_amax, k_mean, k_tail, v_tail, lens, k_new, v_new, new_lens,
                                                   B, Hkv, 0, T, head_dim, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl);
    sage::PagedArgs g;
    if (const int rc = sage::kv_check_pointers(e, p)) return rc;
    if (const int rc = sage::paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    p.cap = max_pages_per_seq * page_size;          // (the logical capacity: at most 2^30, checked above)
    if (const int rc = sage::kv_check_batch(e, B, Hkv)) return rc;
    if (const int rc = sage::kv_check_rows(e, p)) return rc;
    if (const int rc = sage::kv_check_dtype_aligned(e, p, dtype)) return rc;
    if (const int rc = sage::paged_check_table_aligned(e, block_table)) return rc;
    if (const int rc = sage::kv_check_strides(e, p)) return rc;
    const hipError_t err = sage::launch_kvpaged_append(p, g, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return sage::set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
