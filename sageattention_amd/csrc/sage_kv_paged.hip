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

#define KVP_REQUIRE(cond, ...) do { if (!(cond)) return sage::set_last_error(SAGE_EINVAL, __VA_ARGS__); } while (0)

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
    auto a16 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
    KVP_REQUIRE(k_int8 && k_scale && v_image && v_scale && v_amax && k_tail && v_tail && lens,
                "sage_kvpaged_append: null cache pointer (only k_mean may be null)");
    KVP_REQUIRE(k_new && v_new, "sage_kvpaged_append: null k_new / v_new pointer");
    KVP_REQUIRE(block_table, "sage_kvpaged_append: null block_table");
    const int shift = sage::paged_shift(page_size);
    KVP_REQUIRE(shift >= 0, "sage_kvpaged_append: page_size must be 64 * 2^k (got %d)", page_size);
    KVP_REQUIRE(num_pages >= 1, "sage_kvpaged_append: num_pages must be at least 1 (got %d)", num_pages);
    KVP_REQUIRE(max_pages_per_seq >= 1 && (int64_t)max_pages_per_seq * page_size <= ((int64_t)1 << 30) && bt_stride >= max_pages_per_seq,
                "sage_kvpaged_append: max_pages_per_seq must be at least 1, max_pages_per_seq * page_size at most 2^30 and bt_stride at least "
                "max_pages_per_seq (got %d, page_size %d, bt_stride %lld)", max_pages_per_seq, page_size, (long long)bt_stride);
    KVP_REQUIRE(B > 0 && B <= 65535 && Hkv > 0 && Hkv <= 65535, "sage_kvpaged_append: B and Hkv must be in [1, 65535] (got %d, %d)", B, Hkv);
    KVP_REQUIRE(head_dim == 64 || head_dim == 128, "sage_kvpaged_append: head_dim must be 64 or 128 (got %d)", head_dim);
    KVP_REQUIRE(T >= 1, "sage_kvpaged_append: T must be at least 1 (got %d)", T);
    KVP_REQUIRE(dtype == SAGE_DTYPE_F16 || dtype == SAGE_DTYPE_BF16, "sage_kvpaged_append: bad dtype %d", dtype);
    KVP_REQUIRE(a16(k_int8) && a16(k_scale) && a16(v_image) && a16(k_tail) && a16(v_tail) && a16(k_new) && a16(v_new) && (!k_mean || a16(k_mean)),
                "sage_kvpaged_append: k_int8 / k_scale / v_image / k_mean / k_tail / v_tail / k_new / v_new must be 16-byte aligned");
    KVP_REQUIRE((reinterpret_cast<uintptr_t>(block_table) & 3u) == 0, "sage_kvpaged_append: block_table must be 4-byte aligned");
    KVP_REQUIRE(k_sb % 8 == 0 && k_sh % 8 == 0 && k_sl % 8 == 0 && v_sb % 8 == 0 && v_sh % 8 == 0 && v_sl % 8 == 0,
                "sage_kvpaged_append: k_new / v_new strides must be multiples of 8 elements");
    sage::KvCacheParams p{};
    p.k_int8 = k_int8; p.k_scale = k_scale; p.v_image = static_cast<unsigned char *>(v_image); p.v_scale = v_scale; p.v_amax = v_amax;
    p.k_mean = static_cast<const uint16_t *>(k_mean);
    p.k_tail = static_cast<uint16_t *>(k_tail); p.v_tail = static_cast<uint16_t *>(v_tail); p.lens = lens;
    p.k_new = static_cast<const uint16_t *>(k_new); p.v_new = static_cast<const uint16_t *>(v_new); p.new_lens = new_lens;
    p.B = B; p.H = Hkv; p.cap = max_pages_per_seq * page_size; p.T = T; p.D = head_dim;
    p.k_sb = k_sb; p.k_sh = k_sh; p.k_sl = k_sl; p.v_sb = v_sb; p.v_sh = v_sh; p.v_sl = v_sl;
    p.scale_max = 448.0f;
    const sage::PagedArgs g{block_table, (long)bt_stride, shift, num_pages, max_pages_per_seq};
    const hipError_t e = sage::launch_kvpaged_append(p, g, dtype, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return sage::set_last_error(SAGE_ELAUNCH, "sage_kvpaged_append launch: %s", hipGetErrorString(e));
    return SAGE_OK;
}

}  // extern "C"
