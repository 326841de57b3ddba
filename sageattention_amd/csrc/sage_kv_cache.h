// sage_kv_cache.h -- what the appendable cache's two translation units share: the parameter block of its launches and the row range of an append
// (sage_kv_cache.hip: the contiguous cache and the commit launch; sage_kv_paged.hip: the paged pool's append and its C entry points -- a unit of
// its own because kernels added to sage_kv_cache.hip changed the register numbering of the D = 64 kernels already there) -- and, host code
// only, the argument checks their C entries and sage_kvpaged_attn (sage_cabi.hip) have in common, each sentence written once.
#pragma once
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_host_checks.h"

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

// launch 2 of an append (sage_kv_cache.hip): the tails and the lengths, per sample -- the same launch for the contiguous cache and the paged pool
hipError_t launch_kvcache_commit(const KvCacheParams &p, hipStream_t s);

// ---- host side: the argument checks of sage_kvcache_append, sage_kvpaged_append and sage_kvpaged_attn.  `e` is the entry's name, the prefix
// of every message; each function returns SAGE_OK or what the entry returns.  The entries check in different orders (the contiguous append:
// head_dim and T before B / Hkv; the paged one: the page geometry and B / Hkv first, the table's alignment behind the 16-byte alignment), so
// the checks are cut into the runs that stand together in every entry, and an entry calls the runs in its own order.

// the parameter block of an append from the entry's arguments (cap: the capacity, or the logical capacity of a paged sequence)
inline KvCacheParams kv_append_params(int8_t *k_int8, float *k_scale, void *v_image, float *v_scale, const float *v_amax, const void *k_mean,
                                      void *k_tail, void *v_tail, int32_t *lens, const void *k_new, const void *v_new, const int32_t *new_lens,
                                      int B, int Hkv, int cap, int T, int head_dim,
                                      int64_t k_sb, int64_t k_sh, int64_t k_sl, int64_t v_sb, int64_t v_sh, int64_t v_sl)
{
    return KvCacheParams{k_int8, k_scale, static_cast<unsigned char *>(v_image), v_scale, v_amax, static_cast<const uint16_t *>(k_mean),
                         static_cast<uint16_t *>(k_tail), static_cast<uint16_t *>(v_tail), lens,
                         static_cast<const uint16_t *>(k_new), static_cast<const uint16_t *>(v_new), new_lens,
                         B, Hkv, cap, T, head_dim, (long)k_sb, (long)k_sh, (long)k_sl, (long)v_sb, (long)v_sh, (long)v_sl, /* scale_max (e4m3) */ 448.0f};
}

inline int kv_check_pointers(const char *e, const KvCacheParams &p)
{
    SAGE_REQUIRE(p.k_int8 && p.k_scale && p.v_image && p.v_scale && p.v_amax && p.k_tail && p.v_tail && p.lens,
                 "%s: null cache pointer (only k_mean may be null)", e);
    SAGE_REQUIRE(p.k_new && p.v_new, "%s: null k_new / v_new pointer", e);
    return SAGE_OK;
}
inline int kv_check_rows(const char *e, const KvCacheParams &p)
{
    SAGE_REQUIRE(p.D == 64 || p.D == 128, "%s: head_dim must be 64 or 128 (got %d)", e, p.D);
    SAGE_REQUIRE(p.T >= 1, "%s: T must be at least 1 (got %d)", e, p.T);
    return SAGE_OK;
}
inline int kv_check_batch(const char *e, int B, int Hkv)
{
    SAGE_REQUIRE(B > 0 && B <= 65535 && Hkv > 0 && Hkv <= 65535, "%s: B and Hkv must be in [1, 65535] (got %d, %d)", e, B, Hkv);
    return SAGE_OK;
}
inline int kv_check_dtype_aligned(const char *e, const KvCacheParams &p, int dtype)
{
    SAGE_REQUIRE(dtype == SAGE_DTYPE_F16 || dtype == SAGE_DTYPE_BF16, "%s: bad dtype %d", e, dtype);
    SAGE_REQUIRE(aligned16(p.k_int8) && aligned16(p.k_scale) && aligned16(p.v_image) && aligned16(p.k_tail) && aligned16(p.v_tail) &&
                 aligned16(p.k_new) && aligned16(p.v_new) && (!p.k_mean || aligned16(p.k_mean)),
                 "%s: k_int8 / k_scale / v_image / k_mean / k_tail / v_tail / k_new / v_new must be 16-byte aligned", e);
    return SAGE_OK;
}
inline int kv_check_strides(const char *e, const KvCacheParams &p)
{
    SAGE_REQUIRE(multiples_of(8, p.k_sb, p.k_sh, p.k_sl) && multiples_of(8, p.v_sb, p.v_sh, p.v_sl),
                 "%s: k_new / v_new strides must be multiples of 8 elements", e);
    return SAGE_OK;
}

// the page geometry of a paged entry, checked, as the kernels' PagedArgs; the table's alignment, which no entry checks next to it
inline int paged_args(const char *e, const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq, PagedArgs &g)
{
    SAGE_REQUIRE(block_table, "%s: null block_table", e);
    const int shift = paged_shift(page_size);
    SAGE_REQUIRE(shift >= 0, "%s: page_size must be 64 * 2^k (got %d)", e, page_size);
    SAGE_REQUIRE(num_pages >= 1, "%s: num_pages must be at least 1 (got %d)", e, num_pages);
    SAGE_REQUIRE(max_pages_per_seq >= 1 && (int64_t)max_pages_per_seq * page_size <= ((int64_t)1 << 30) && bt_stride >= max_pages_per_seq,
                 "%s: max_pages_per_seq must be at least 1, max_pages_per_seq * page_size at most 2^30 and bt_stride at least "
                 "max_pages_per_seq (got %d, page_size %d, bt_stride %lld)", e, max_pages_per_seq, page_size, (long long)bt_stride);
    g = PagedArgs{block_table, (long)bt_stride, shift, num_pages, max_pages_per_seq};
    return SAGE_OK;
}
inline int paged_check_table_aligned(const char *e, const int32_t *block_table)
{
    SAGE_REQUIRE((reinterpret_cast<uintptr_t>(block_table) & 3u) == 0, "%s: block_table must be 4-byte aligned", e);
    return SAGE_OK;
}

}  // namespace sage
