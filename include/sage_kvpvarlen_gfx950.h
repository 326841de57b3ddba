/*
 * sage_kvpvarlen_gfx950.h -- C ABI of the PACKED, variable-length calls on the paged quantised KV cache of libsage_gfx950.so (AMD MI355X,
 * gfx950 / CDNA4).
 *
 * include/sage_kvpaged_gfx950.h takes dense operands with one length for all: q [B, Hq, Lq, D], new rows [B, Hkv, T, D].  A continuous-batching
 * step holds one row for each decoding sequence, a few hundred for each prefill chunk and none for an idle slot, packed as [total, H, D] behind a
 * prefix array.  These entries are that header's two calls on such operands:
 *
 *  cu_seqlens   int32 [B + 1] in device memory, written by the caller: sample b owns rows cu_seqlens[b] .. cu_seqlens[b + 1] - 1 of the packed
 *               tensor.  `total` are the rows the packed tensor has; `max_seqlen_q` / `max_new` the most rows a sample gets in this call -- host
 *               ints that size the grid (rows of a sample beyond them are not computed / not appended).
 *
 * Device rule -- a bad prefix array gives wrong numbers, never an access outside the packed tensors: both words of a sample are clamped on the
 * device, 0 <= first <= first + rows <= total and rows <= the maximum, before anything is formed from them (csrc/sage_ragged.h).  Nothing is
 * read on the host; grids follow from the shapes and the two maxima alone, so append plus attention capture into a HIP graph and a replay follows
 * the prefix arrays', the lengths' and the table's contents.
 *
 * Per work item the attention kernel runs what sage_kvpaged_attn runs for a call of that sample's own row count, and the append writes what
 * sage_kvpaged_append writes for the zero-padded rows with new_lens: the results are bit for bit those.
 *
 * Conventions as in include/sage_gfx950.h and include/sage_kvpaged_gfx950.h (both unchanged, as are their ABI versions): caller-owned buffers,
 * strides in ELEMENTS; 0 or a negative code (-1: bad argument, -2: launch error), message in sage_last_error().  Argument errors return -1 before
 * anything touches a GPU.
 * Replaces in the reference: nothing (thu-ml/SageAttention has no KV cache).
 */
#ifndef SAGE_KVPVARLEN_GFX950_H
#define SAGE_KVPVARLEN_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_KVPVARLEN_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_KVPVARLEN_API __attribute__((visibility("default")))
#else
#define SAGE_KVPVARLEN_API
#endif

SAGE_KVPVARLEN_API int sage_kvpvarlen_abi_version(void);

/*
 * sage_kvpaged_attn over packed query rows: q fp16 / bf16 [total_q, Hq, D] by its row and head strides (q_sl, q_sh), o likewise, lse nullable
 * fp32 [Hq, total_q] with head stride lse_sh (log2 units); the pool, the table, v_scale [B, Hkv, D] and kv_lens [B] as there.  The call is
 * causal (is_causal must be 1) and SageLaunchAttr.q_start is REQUIRED: row i of sample b stands at key q_start[b] + i (clamped to
 * [-rows_b, capacity]); the bottom-right alignment is q_start[b] = kv_lens[b] - rows_b.  SageLaunchAttr.window and grid_out mean what they
 * mean there.  The grid is B * Hq * ceil(max_seqlen_q / 128) workgroups; one past a sample's last row leaves at once.
 * Checked in this order: null tensors, null kv_lens, null cu_seqlens_q, the page geometry, B / Hkv, the table's alignment, cu_seqlens_q's
 * alignment, total_q / max_seqlen_q >= 1, is_causal, the grid's size, lse_sh; then, refused by name as in sage_kvpaged_attn,
 * SAGE_ATTR_KV_SPLIT, SAGE_ATTR_FP8_FOLDED_SCORES, SAGE_ATTR_FORCE_PERSISTENT, and here SAGE_ATTR_GQA_PACK; a missing q_start; then that entry's
 * checks of head_dim, Hq / Hkv, dtypes, alignment and strides.
 */
SAGE_KVPVARLEN_API int sage_kvpvarlen_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
                                           const float *k_scale, const float *v_scale, const int32_t *kv_lens, const int32_t *cu_seqlens_q,
                                           const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                           int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                                           int64_t q_sl, int64_t q_sh, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                           int64_t o_sl, int64_t o_sh, int64_t lse_sh,
                                           int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr);

/*
 * sage_kvpaged_append of packed new rows: k_new / v_new fp16 / bf16 [total, Hkv, D] by their row and head strides; sample b takes its
 * min(cu_seqlens[b + 1] - cu_seqlens[b], max_new) rows from row cu_seqlens[b] on (clamped as above), then what still fits into the logical
 * capacity.  Two launches of (ceil((63 + max_new) / 64), Hkv, B) and (B) workgroups; everything else is that entry's.
 * Checked in this order: the cache's and the new rows' pointers, null cu_seqlens, the page geometry, B / Hkv, head_dim and max_new >= 1,
 * total >= 1, dtype and 16-byte alignment, the table's and cu_seqlens's alignment, strides.
 */
SAGE_KVPVARLEN_API int sage_kvpvarlen_append(int8_t *k_int8, float *k_scale, void *v_image, float *v_scale, const float *v_amax, const void *k_mean,
                                             void *k_tail, void *v_tail, int32_t *lens,
                                             const void *k_new, const void *v_new, const int32_t *cu_seqlens,
                                             int B, int Hkv, int total, int max_new, int head_dim,
                                             int64_t k_sl, int64_t k_sh, int64_t v_sl, int64_t v_sh,
                                             int dtype,
                                             const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                             void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_KVPVARLEN_GFX950_H */
