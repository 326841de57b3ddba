/*
 * sage_kvfork_gfx950.h -- C ABI of the FORK of sequences of the paged quantised KV cache of libsage_gfx950.so (AMD MI355X, gfx950 / CDNA4).
 *
 * include/sage_kvpaged_gfx950.h keeps the quantised keys and values of B sequence slots in a pool of pages behind a block table.  What a block
 * table buys a serving stack is SHARING: one system prompt under many requests, n > 1 samples of one prompt, beam search, a scratch copy of a
 * sequence to verify draft tokens on.  sage_kvfork makes a second sequence out of a first without touching raw rows: the child's table names
 * the parent's closed pages, the parent's open page is copied into a page of the child's own, and the child takes the parent's per-slot state.
 *
 * Why the shared pages are exact: the child takes the parent's FROZEN statistics (k_mean, v_amax).  With frozen statistics the bytes of a
 * 64-key block depend on that block's rows alone (include/sage_kvcache_gfx950.h), so every closed block of the parent is, byte for byte, what
 * the child would have produced from the same rows.  Attention only reads through the table; an append writes only blocks >= lens[b] / 64 --
 * neither changes.  After a fork the two sequences append independently: the open page was copied, so neither writes a page the other reads.
 *
 * Semantics, all on the device, per fork i of n:  s = src_slots[i], d = dst_slots[i], pg = new_pages[i], page size ps = 64 << k,
 * cap = max_pages_per_seq * ps.
 *  L = clamp(lens[s], 0, cap).
 *  P = L when prefix_lens is null; otherwise P = clamp(prefix_lens[i], 0, L), and if P < L then P &= ~63: A PREFIX SHORTER THAN THE PARENT IS
 *      ROUNDED DOWN TO A BLOCK BOUNDARY (a multiple of 64 keys).  Only there are the parent's bytes exactly the prefix's own: the parent's
 *      open block was quantised over more rows than the prefix holds, and the raw rows of a closed block are gone.
 *  np = P >> (6 + k) whole pages are shared; r = P & (ps - 1) keys lie in the open page.
 *  The fork is SKIPPED ENTIRELY when s or d lies outside [0, B) or s == d.  Otherwise
 *  * table:  block_table[d][0 : np] = block_table[s][0 : np], raw ids as they stand; if np < max_pages_per_seq, block_table[d][np] = pg, as
 *            given even when it is no page of the pool (the child's first own page).  Entries behind it are untouched.
 *  * copy-on-write of the open page:  if r > 0, tiles [0, ceil(r / 64)) of page block_table[s][np] are copied to page pg -- a tile is 64 INT8
 *            rows, 4 scale slots and one V tile, for every kv-head -- but only if both ids lie in [0, num_pages); otherwise nothing of the pool
 *            is written (sage_kvpaged_append's rule).  No other pool byte is written.
 *  * per-slot state:  v_scale, v_amax, k_mean (where non-null) of d become those of s; rows [0, P % 64) of k_tail / v_tail are copied, the
 *            other tail rows are untouched; lens[d] = P.
 *
 * The caller's contract, documented and not detected: dst_slots are distinct and disjoint from src_slots (one source may fork to many
 * destinations in one call); new_pages are distinct and named by no live table entry.  A violation gives wrong numbers, never an access
 * outside a tensor.  There is no allocator and there are no reference counts here: which pages are free, and when a shared page may be
 * reused, is the caller's to know.
 *
 * Draft verification (speculative decoding) without truncating a cache -- which would not be sound, the raw rows of a closed block are gone:
 * fork the sequence into a scratch slot, append the k draft rows to the scratch slot, attend with Lq = k and the bottom-right causal mask on
 * the scratch slot, append the accepted rows to the original.
 *
 * Conventions as in include/sage_gfx950.h (SAGE_ABI_VERSION, SAGE_KVCACHE_ABI_VERSION and SAGE_KVPAGED_ABI_VERSION are untouched):
 * caller-owned buffers, no state, no allocation, no host read of any tensor, no atomics, no synchronisation; ONE launch whose grid follows
 * from the shapes alone -- a fork captures into a HIP graph and a replay follows the contents of the index arrays, the lengths and the table.
 * 0 or a negative code (-1: bad argument, -2: launch error), message in sage_last_error().  Argument errors return -1 before anything touches
 * a GPU.
 * Replaces in the reference: nothing (thu-ml/SageAttention has no KV cache).
 */
#ifndef SAGE_KVFORK_GFX950_H
#define SAGE_KVFORK_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_KVFORK_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_KVFORK_API __attribute__((visibility("default")))
#else
#define SAGE_KVFORK_API
#endif

SAGE_KVFORK_API int sage_kvfork_abi_version(void);

/*
 * n forks in one launch.  k_int8 / k_scale / v_image: the pool of include/sage_kvpaged_gfx950.h; v_scale, v_amax fp32 [B, Hkv, head_dim],
 * k_mean (nullable) [B, Hkv, head_dim] and k_tail / v_tail [B, Hkv, 64, head_dim] in `dtype` (SAGE_DTYPE_F16 / SAGE_DTYPE_BF16), lens int32
 * [B]: the per-slot state, read at the sources and WRITTEN at the destinations (v_amax and k_mean included); block_table int32
 * [B, max_pages_per_seq], row stride bt_stride elements, read at the sources and written at the destinations.  src_slots, dst_slots,
 * new_pages int32 [n] and prefix_lens (nullable) int32 [n] in device memory.
 * Argument errors: a null pointer where one is required (only k_mean and prefix_lens may be null), page_size not 64 * 2^k, num_pages /
 * max_pages_per_seq / bt_stride as in sage_kvpaged_append, B or Hkv outside [1, 65535], head_dim not 64 or 128, dtype, k_int8 / k_scale /
 * v_image / k_mean / k_tail / v_tail not 16-byte aligned, block_table / src_slots / dst_slots / new_pages / prefix_lens not 4-byte aligned,
 * n outside [1, 65535].
 */
SAGE_KVFORK_API int sage_kvfork(int8_t *k_int8, float *k_scale, void *v_image, float *v_scale, float *v_amax, void *k_mean,
                                void *k_tail, void *v_tail, int32_t *lens,
                                int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                int B, int Hkv, int head_dim, int dtype,
                                const int32_t *src_slots, const int32_t *dst_slots, const int32_t *new_pages, const int32_t *prefix_lens,
                                int n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_KVFORK_GFX950_H */
