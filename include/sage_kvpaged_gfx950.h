/*
 * sage_kvpaged_gfx950.h -- C ABI of the PAGED quantised KV cache of libsage_gfx950.so (AMD MI355X, gfx950 / CDNA4).
 *
 * include/sage_kvcache_gfx950.h keeps every sequence's quantised keys and values in one contiguous slab of `capacity` rows.  A serving stack
 * allocates its KV memory in pages and hands the attention call a block table; these entries are the same cache over such a pool.
 *
 * The POOL is `num_pages` pages of `page_size` = 64 * 2^k keys (k >= 0: whole 64-key tiles, and a shift instead of a division), laid out exactly
 * as the cache of sage_kvcache_gfx950.h with B = num_pages and capacity = page_size:
 *  k_int8   int8  [num_pages, Hkv, page_size, head_dim]
 *  k_scale  fp32  [num_pages, Hkv, page_size / 64 * 4]
 *  v_image  uint8 [num_pages, Hkv, page_size / 64, head_dim, 64]
 * Per SEQUENCE, for B slots, the state is that header's, unchanged: v_scale, v_amax, k_mean [B, Hkv, head_dim], k_tail / v_tail
 * [B, Hkv, 64, head_dim], lens int32 [B].
 *
 *  block_table  int32 [B, max_pages_per_seq] in device memory, row stride `bt_stride` elements, written by the caller: logical 64-key tile t of
 *               sample b lies in page block_table[b][t >> k], at tile t & (2^k - 1) of that page.  The logical capacity of a sequence is
 *               max_pages_per_seq * page_size; it stands where Lk / capacity stand in the two headers above (the q_start clamps, the window
 *               clamp, the dropping of rows that do not fit).
 *
 * Device rules -- a bad table gives wrong numbers, never an access outside the pool:
 *  * sage_kvpaged_attn reads the table entries of tiles < ceil(len_b / 64) and no others (a window additionally skips the tiles in front of the
 *    window's first tile); entries behind them may hold anything; a sample without keys reads none (o = 0, lse = -inf).  Every id read is
 *    clamped to [0, num_pages - 1] on the scalar unit before it forms an address.
 *  * sage_kvpaged_append does not write a block whose page id lies outside [0, num_pages): neither k_int8 nor k_scale nor v_image.  `lens`
 *    still advance (the commit launch does not look at the table).  Two sequences that append into one page are the caller's error; it is
 *    not detected.
 *
 * With frozen statistics a row's bytes depend on its own 64-key block alone, and the attention kernels fetch K, the V image and the K scales one
 * 64-key tile at a time: "which tile" is a table lookup and the arithmetic is untouched.  A paged cache holds, at the places the table names,
 * byte for byte what the contiguous cache holds, and sage_kvpaged_attn returns bit for bit what sage_attn_fused_q_pv_f8_kvlens returns on it.
 *
 * Conventions as in include/sage_gfx950.h (unchanged; SAGE_ABI_VERSION and SAGE_KVCACHE_ABI_VERSION are untouched): caller-owned buffers, no
 * state, no allocation, no host read of any tensor, no synchronisation, grids from the shapes alone -- append plus attention capture into a HIP
 * graph and a replay follows the table's contents.  Strides in ELEMENTS; 0 or a negative code (-1: bad argument, -2: launch error), message in
 * sage_last_error().  Argument errors return -1 before anything touches a GPU.
 * Replaces in the reference: nothing (thu-ml/SageAttention has no KV cache).
 */
#ifndef SAGE_KVPAGED_GFX950_H
#define SAGE_KVPAGED_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_KVPAGED_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_KVPAGED_API __attribute__((visibility("default")))
#else
#define SAGE_KVPAGED_API
#endif

SAGE_KVPAGED_API int sage_kvpaged_abi_version(void);

/*
 * sage_kvcache_append on a pool: the first seventeen arguments mean what they mean there, with k_int8 / k_scale / v_image the pool's tensors
 * and the logical capacity max_pages_per_seq * page_size in place of `capacity`; workgroup (j, h, b) of launch 1 owns logical block
 * lens[b] / 64 + j and writes its INT8 rows, four scales and V tile at the block's place in the page the table names -- or nothing, when the id
 * is not a page of the pool.  v_scale, the tails, lens and launch 2 are per sequence, as they are there.
 * Argument errors: a null pointer where one is required (only k_mean and new_lens may be null), page_size not 64 * 2^k, num_pages /
 * max_pages_per_seq / B / Hkv out of range (B, Hkv in [1, 65535]; num_pages >= 1; 1 <= max_pages_per_seq * page_size <= 2^30; bt_stride >=
 * max_pages_per_seq), head_dim, T < 1, alignment, strides, dtype.
 */
SAGE_KVPAGED_API int sage_kvpaged_append(int8_t *k_int8, float *k_scale, void *v_image, float *v_scale, const float *v_amax, const void *k_mean,
                                         void *k_tail, void *v_tail, int32_t *lens,
                                         const void *k_new, const void *v_new, const int32_t *new_lens,
                                         int B, int Hkv, int T, int head_dim,
                                         int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                         int64_t v_sb, int64_t v_sh, int64_t v_sl,
                                         int dtype,
                                         const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                         void *stream);

/*
 * sage_attn_fused_q_pv_f8_kvlens (include/sage_gfx950.h) on a pool: q fp16 / bf16 [B, Hq, Lq, D] by strides, o likewise, lse nullable
 * [B, Hq, Lq] (log2 units), k / v_image / k_scale the pool's tensors (k_sb: the PAGE stride of k, k_sh / k_sl its head and row strides: the
 * head-major pool and its NHD view both fit), v_scale [B, Hkv, D] and kv_lens [B] per sequence.  The padded key length of the call is
 * max_pages_per_seq * page_size.  `attr` is that entry's SageLaunchAttr with the same meaning of q_start, window, SAGE_ATTR_GQA_PACK and
 * grid_out; the grid is the unpaged call's.  Refused by name: SAGE_ATTR_KV_SPLIT (pass 1 and the split's kernels do not look pages up), the
 * folded score form (SAGE_ATTR_FP8_FOLDED_SCORES) and SAGE_ATTR_FORCE_PERSISTENT (a paged launch takes the ordinary dispatch; a launch
 * workspace is accepted and ignored).  The exact split on a pool is an entry of its own, sage_kvpsplit_attn (include/sage_kvpsplit_gfx950.h),
 * with this argument list.
 */
SAGE_KVPAGED_API int sage_kvpaged_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
                                       const float *k_scale, const float *v_scale, const int32_t *kv_lens,
                                       const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                       int B, int Hq, int Hkv, int Lq, int D,
                                       int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                       int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                       int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_KVPAGED_GFX950_H */
