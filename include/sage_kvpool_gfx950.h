/*
 * sage_kvpool_gfx950.h -- C ABI of the PAGE POOL of the paged quantised KV cache of libsage_gfx950.so (AMD MI355X, gfx950 / CDNA4): a free
 * stack, a reference count per page and the block table, kept on the device.
 *
 * include/sage_kvpaged_gfx950.h reads a block table the caller wrote, and include/sage_kvfork_gfx950.h takes the child's page from the caller:
 * which pages are free, and when a shared page may be reused, was the caller's to know -- on the host, between two launches.  The entries here
 * keep that knowledge in one caller-owned int32 workspace and move it by what lens, new_lens / cu_seqlens and the index arrays hold when the
 * launch runs: ONE small launch in front of an append (reserve), of a fork (fork_prepare), or on its own (release).  A captured
 * reserve -> append -> attend step then replays across page boundaries without the host.
 *
 * The workspace (pool_ws, sage_kvpool_ws_bytes(num_pages, B) = 4 * (16 + 2 * num_pages + B) bytes):
 *   hdr[16]               hdr[0] = n_free; hdr[1] = the slots (forks) the last reserve (fork_prepare) refused; hdr[2] = the pages that call was
 *                         short of, max(0, pages asked for - n_free) if it refused any, else 0; hdr[3] = refusals since init; the rest 0.
 *   free_stack[num_pages] the free pages; free_stack[n_free - 1] is handed out next.
 *   refcount[num_pages]   table entries that hold a reference to the page.
 *   n_owned[B]            the leading entries of block_table[b] that hold a reference (a forked child owns a first page of its own even when its
 *                         prefix ends on a page boundary, so ceil(lens / page_size) does not tell it).
 * ps = page_size, mp = max_pages_per_seq, cap = mp * ps.
 *
 * init       every page free, page 0 on top (free_stack[i] = num_pages - 1 - i), every count and n_owned 0.  The table must be its -1 fill.
 * reserve    n_b = clamp(new_lens[b], 0, T), or sage_kvpvarlen_append's clamp of (cu_seqlens[b], cu_seqlens[b + 1]) to total and max_new;
 *            L = clamp(lens[b], 0, cap); want_b = ceil(min(L + n_b, cap) / ps); need_b = n_b > 0 ? max(0, want_b - clamp(n_owned[b], 0, mp)) : 0.
 *            Slot b is GRANTED iff need_b == 0 or need_0 + .. + need_b <= n_free: refused slots' needs count, so the granted slots with a need
 *            are a prefix of the slots with a need.  A granted slot with a need pops its pages from the top of the stack, slots in ascending
 *            order, entries in ascending order into block_table[b][n_owned[b] ..], each with refcount 1; n_owned[b] = want_b.  granted[b] = n_b
 *            for a granted slot and 0 for a refused one, whose table row and n_owned stay.  hdr[0 .. 3] are updated.
 * release    every listed slot b in [0, B): each entry e < clamp(n_owned[b], 0, mp) whose id lies in [0, num_pages) loses one reference, the
 *            entries become -1, n_owned[b] = 0, lens[b] = 0.  The pages whose count reached 0 in this call are pushed once each, highest id
 *            first: the lowest freed id is handed out next, whatever the order of execution.  Two listed slots may share pages; the slots are
 *            distinct (the caller's contract).  hdr[0] is updated, hdr[1 .. 3] stay.
 * fork_prepare   for fork i with s = src_slots[i], d = dst_slots[i]: P and np = P / ps as include/sage_kvfork_gfx950.h states them.  REFUSED
 *            if s or d lies outside [0, B), s == d, n_owned[d] != 0, or it needs a page (np < mp) and the forks 0 .. i that need one ask for
 *            more than n_free (reserve's rule).  A granted fork adds one reference to every id in [0, num_pages) among block_table[s][0 : np],
 *            pops new_pages[i] (refcount 1; -1 if np == mp), sets n_owned[d] = np + (np < mp) and dst_eff[i] = d.  A refused fork writes
 *            dst_eff[i] = new_pages[i] = -1: sage_kvfork, given dst_eff for dst_slots, then skips it entirely.  Contract as sage_kvfork's:
 *            dst_slots distinct and disjoint from src_slots.  hdr[0 .. 3] are updated.
 *
 * Device rule: every word is clamped before anything is formed from it -- n_free to [0, num_pages], a popped word to [0, num_pages - 1],
 * n_owned to [0, mp], table ids checked, sums in 64 bits.  A workspace init never wrote gives wrong numbers, never an access outside pool_ws,
 * block_table, lens, granted, new_pages or dst_eff, and no table entry the pool writes lies outside [0, num_pages).
 *
 * Conventions as in include/sage_gfx950.h (the other seven headers and their ABI versions are untouched): caller-owned buffers, no
 * allocation, no host read of any array, no synchronisation; one launch of one workgroup on the caller's stream (init: a few), graph-capturable.
 * 0 or a negative code (-1: bad argument, -2: launch error), message in sage_last_error() under the entry's name.  Argument errors return -1
 * before anything touches a GPU, checked in this order: the page geometry as sage_kvpaged_append checks it (null block_table, page_size not
 * 64 * 2^k, num_pages < 1, max_pages_per_seq / bt_stride); null pointers (reserve: exactly one of new_lens and cu_seqlens is non-null); 4-byte
 * alignment of every int array; B outside [1, sage_varlen_plan_max_seqs()], then n outside the same range, then T (or total, max_new) < 1; the
 * workspace smaller than sage_kvpool_ws_bytes(num_pages, B).  (init has no table: num_pages, null, alignment, B, the workspace.)
 * The *_host twins run the same functions (csrc/sage_page_pool.h) on HOST arrays, no GPU; arguments and checks are the device entries'.
 * Replaces in the reference: nothing (thu-ml/SageAttention has no KV cache).
 */
#ifndef SAGE_KVPOOL_GFX950_H
#define SAGE_KVPOOL_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_KVPOOL_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_KVPOOL_API __attribute__((visibility("default")))
#else
#define SAGE_KVPOOL_API
#endif

SAGE_KVPOOL_API int sage_kvpool_abi_version(void);

/* bytes of the workspace: 4 * (16 + 2 * num_pages + B); -1 for num_pages < 1 or B < 1 */
SAGE_KVPOOL_API int64_t sage_kvpool_ws_bytes(int num_pages, int B);

SAGE_KVPOOL_API int sage_kvpool_init(int32_t *pool_ws, int64_t pool_ws_bytes, int num_pages, int B, void *stream);
SAGE_KVPOOL_API int sage_kvpool_init_host(int32_t *pool_ws, int64_t pool_ws_bytes, int num_pages, int B);

/* block_table int32 [B, max_pages_per_seq] (row stride bt_stride elements), lens [B], new_lens [B] or cu_seqlens [B + 1], granted [B] */
SAGE_KVPOOL_API int sage_kvpool_reserve(int32_t *pool_ws, int64_t pool_ws_bytes, int32_t *block_table, int64_t bt_stride, int num_pages, int page_size,
                                        int max_pages_per_seq, int B, const int32_t *lens, const int32_t *new_lens, int T,
                                        const int32_t *cu_seqlens, int total, int max_new, int32_t *granted, void *stream);
SAGE_KVPOOL_API int sage_kvpool_reserve_host(int32_t *pool_ws, int64_t pool_ws_bytes, int32_t *block_table, int64_t bt_stride, int num_pages, int page_size,
                                             int max_pages_per_seq, int B, const int32_t *lens, const int32_t *new_lens, int T,
                                             const int32_t *cu_seqlens, int total, int max_new, int32_t *granted);

/* slots int32 [n] */
SAGE_KVPOOL_API int sage_kvpool_release(int32_t *pool_ws, int64_t pool_ws_bytes, int32_t *block_table, int64_t bt_stride, int num_pages, int page_size,
                                        int max_pages_per_seq, int B, int32_t *lens, const int32_t *slots, int n, void *stream);
SAGE_KVPOOL_API int sage_kvpool_release_host(int32_t *pool_ws, int64_t pool_ws_bytes, int32_t *block_table, int64_t bt_stride, int num_pages, int page_size,
                                             int max_pages_per_seq, int B, int32_t *lens, const int32_t *slots, int n);

/* src_slots, dst_slots, prefix_lens (nullable), new_pages, dst_eff int32 [n]; the table and lens are read, sage_kvfork writes them afterwards */
SAGE_KVPOOL_API int sage_kvpool_fork_prepare(int32_t *pool_ws, int64_t pool_ws_bytes, const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size,
                                             int max_pages_per_seq, int B, const int32_t *lens, const int32_t *src_slots, const int32_t *dst_slots,
                                             const int32_t *prefix_lens, int n, int32_t *new_pages, int32_t *dst_eff, void *stream);
SAGE_KVPOOL_API int sage_kvpool_fork_prepare_host(int32_t *pool_ws, int64_t pool_ws_bytes, const int32_t *block_table, int64_t bt_stride, int num_pages,
                                                  int page_size, int max_pages_per_seq, int B, const int32_t *lens, const int32_t *src_slots,
                                                  const int32_t *dst_slots, const int32_t *prefix_lens, int n, int32_t *new_pages, int32_t *dst_eff);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_KVPOOL_GFX950_H */
