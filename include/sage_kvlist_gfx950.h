/*
 * sage_kvlist_gfx950.h -- C ABI of the LISTED step call on the paged quantised KV cache of libsage_gfx950.so (AMD MI355X, gfx950 / CDNA4):
 * include/sage_kvstep_gfx950.h's call with its two launches taking their work items from device-built lists, heaviest first.
 *
 * sage_kvstep_attn launches the decode kernels over B * Hkv * ceil(group / 4) items and the chunk kernels over B * Hq * ceil(max_seqlen_q / 128),
 * both dealt to the eight XCDs as one contiguous run each: the chunk sequences of a step -- or its long decode contexts -- that sit in adjacent
 * slots are one XCD's work while the others idle.  This entry puts one small launch in front that sorts the step on the device:
 *
 *  decode list   the sequences of 1 .. 32 rows, by ceil(keys up to the last row's diagonal / 64) descending; units (list rank, kv head) go to the
 *                XCDs round-robin, the ceil(group / 4) blocks of a unit stay on one XCD;
 *  chunk list    every (sequence, 128-row query block) of the sequences of more rows, by the 64-key tiles the block visits descending: the
 *                launch is a dense launch over Hq heads of that many items (the packed route's work order), sized by a host-known bound,
 *                min(B * ceil(max_seqlen_q / 128), total_q / 128 + min(B, total_q / 33)).
 *
 * Three launches on the caller's stream -- plan, decode kernels, chunk kernels (only if max_seqlen_q > 32 and total_q > 32: host-known facts, the
 * bound is 0 otherwise) -- nothing is read on the host and
 * nothing synchronises: the call captures into a HIP graph, and a replay sorts by what the arrays hold then.  Every row is bit for bit what
 * sage_kvstep_attn writes for the same operands; rows no sequence owns are not written.  The lists order work and nothing else: the kernels read
 * the prefix words again and decide as sage_kvstep_attn's do.
 *
 * The workspace (list_ws, caller-owned int32 device memory, sage_kvlist_ws_bytes) holds hdr[16] = {n_decode, n_chunk_items, group, fold, left,
 * chunk items before the clamp, max key count of a chunk sequence, 0 ...}, decode_list[B] and chunk_items[2 * bound] as (sequence, query block)
 * pairs; entries past the two counts are not written.
 *
 * Device rule as in include/sage_kvpvarlen_gfx950.h, extended to the list: a bad prefix array gives wrong numbers or dropped work, never an access
 * outside the operands or the workspace (a malformed array that yields more chunk items than the bound is clamped to it), and the kernels clamp
 * every list word before they form anything from it, so a workspace the plan never wrote does not reach outside the operands either.
 *
 * Conventions as in include/sage_gfx950.h and include/sage_kvstep_gfx950.h (both unchanged, as are their ABI versions): caller-owned buffers,
 * strides in ELEMENTS; 0 or a negative code (-1: bad argument, -2: launch error), message in sage_last_error().  Argument errors return -1 before
 * anything touches a GPU.
 * Replaces in the reference: nothing (thu-ml/SageAttention has no KV cache).
 */
#ifndef SAGE_KVLIST_GFX950_H
#define SAGE_KVLIST_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_KVLIST_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_KVLIST_API __attribute__((visibility("default")))
#else
#define SAGE_KVLIST_API
#endif

SAGE_KVLIST_API int sage_kvlist_abi_version(void);

/* bytes of the workspace of a call with these three host-known numbers: 4 * (16 + B + 2 * bound); -1 for B < 1, total_q < 1 or max_seqlen_q < 1 */
SAGE_KVLIST_API int64_t sage_kvlist_ws_bytes(int B, int total_q, int max_seqlen_q);

/*
 * The plan launch alone, on `stream`: cu_seqlens_q [B + 1], kv_lens [B] and q_start [B] int32 in device memory, capacity = max_pages_per_seq *
 * page_size, window as SageLaunchAttr.window (0: none); Hq, Hkv and D shape the chunk launch's plan (group, fold, left).  B at most
 * sage_varlen_plan_max_seqs().  -1: a null or misaligned array, B / total_q / max_seqlen_q / capacity < 1, window < 0, Hq % Hkv, D, the workspace.
 */
SAGE_KVLIST_API int sage_kvlist_plan(const int32_t *cu_seqlens_q, const int32_t *kv_lens, const int32_t *q_start,
                                     int B, int total_q, int max_seqlen_q, int capacity, int window, int Hq, int Hkv, int D,
                                     int32_t *list_ws, int64_t list_ws_bytes, void *stream);

/*
 * The same functions on HOST arrays, no GPU: list_ws (host memory, sage_kvlist_ws_bytes) receives what the plan launch writes, decode_grid and
 * chunk_grid (nullable) the workgroups of the two attention launches -- 8 * ceil(B * Hkv / 8) * ceil(Hq / Hkv / 4), and the chunk launch's
 * 8 * ((Hq % 8) * ceil(bound / 8) + (Hq / 8) * bound), 0 if max_seqlen_q <= 32.  The arguments and their checks are sage_kvlist_plan's.
 */
SAGE_KVLIST_API int sage_kvlist_plan_host(const int32_t *cu_seqlens_q, const int32_t *kv_lens, const int32_t *q_start,
                                          int B, int total_q, int max_seqlen_q, int capacity, int window, int Hq, int Hkv, int D,
                                          int32_t *list_ws, int64_t list_ws_bytes, int *decode_grid, int *chunk_grid);

/*
 * sage_kvstep_attn's arguments, argument for argument, with its meanings, followed by the workspace.  SageLaunchAttr.grid_out receives the sum of
 * the two attention grids (sage_kvlist_plan_host's).  A failure of a launch returns without the launches behind it.
 * Checked in sage_kvstep_attn's order, under this entry's name; then the workspace -- null or not 4-byte aligned, fewer bytes than
 * sage_kvlist_ws_bytes(B, total_q, max_seqlen_q) -- and B > sage_varlen_plan_max_seqs().
 */
SAGE_KVLIST_API int sage_kvlist_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
                                     const float *k_scale, const float *v_scale, const int32_t *kv_lens, const int32_t *cu_seqlens_q,
                                     const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                     int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                                     int64_t q_sl, int64_t q_sh, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                     int64_t o_sl, int64_t o_sh, int64_t lse_sh,
                                     int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr,
                                     int32_t *list_ws, int64_t list_ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_KVLIST_GFX950_H */
