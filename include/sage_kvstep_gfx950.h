/*
 * sage_kvstep_gfx950.h -- C ABI of the STEP call on the paged quantised KV cache of libsage_gfx950.so (AMD MI355X, gfx950 / CDNA4): the one
 * attention call a continuous-batching engine makes per step.
 *
 * include/sage_kvpvarlen_gfx950.h attends packed query rows [total_q, Hq, D] behind a prefix array to the paged cache, one workgroup per
 * (sample, query head, block of 128 rows): a decoding sample's single row costs Hq workgroups that each stream the sample's K / V alone.  This
 * entry takes the same operands and sorts the samples on the device, by the row count n_b = min(cu[b + 1] - cu[b], max_seqlen_q) its two prefix
 * words give after the clamps of csrc/sage_ragged.h:
 *
 *  1 <= n_b <= 32   a DECODE sample: the query heads of a GQA group run four to a workgroup over one K / V stream (the work item of
 *                   SAGE_ATTR_GQA_PACK, B * Hkv * ceil(group / 4) workgroups);
 *  n_b > 32         a CHUNK sample: the 128-row kernel of sage_kvpvarlen_attn, its grid and work order;
 *  n_b == 0         idle.
 *
 * Two launches on the caller's stream -- the decode kernels always, the chunk kernels only if max_seqlen_q > 32, a host-known fact, so a pure
 * decode step is one launch -- each over its whole grid, a workgroup whose sample lies outside the launch's band leaving after two scalar loads.
 * Nothing is read on the host and nothing synchronises: the call captures into a HIP graph, and a replay sorts by the prefix array's contents.
 * Every row is bit for bit what sage_kvpvarlen_attn writes for the same operands; rows no sample owns are not written.
 *
 * Device rule as in include/sage_kvpvarlen_gfx950.h: a bad prefix array gives wrong numbers, never an access outside the packed tensors, and no
 * row is written by both launches (the bands partition the clamped counts).
 *
 * Conventions as in include/sage_gfx950.h and include/sage_kvpvarlen_gfx950.h (both unchanged, as are their ABI versions): caller-owned buffers,
 * strides in ELEMENTS; 0 or a negative code (-1: bad argument, -2: launch error), message in sage_last_error().  Argument errors return -1 before
 * anything touches a GPU.
 * Replaces in the reference: nothing (thu-ml/SageAttention has no KV cache).
 */
#ifndef SAGE_KVSTEP_GFX950_H
#define SAGE_KVSTEP_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_KVSTEP_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_KVSTEP_API __attribute__((visibility("default")))
#else
#define SAGE_KVSTEP_API
#endif

SAGE_KVSTEP_API int sage_kvstep_abi_version(void);

/*
 * sage_kvpvarlen_attn's arguments, argument for argument, with its meanings: q / o fp16 / bf16 [total_q, Hq, D] by row and head strides, lse
 * nullable fp32 [Hq, total_q] with head stride lse_sh (log2 units), the pool, the table, v_scale and kv_lens as there; is_causal must be 1 and
 * SageLaunchAttr.q_start is REQUIRED; SageLaunchAttr.window means what it means there.  Hq / Hkv must be at least 2.  SageLaunchAttr.grid_out
 * receives the sum of the workgroups launched: B * Hkv * ceil(Hq / Hkv / 4), plus B * Hq * ceil(max_seqlen_q / 128) when max_seqlen_q > 32.
 * A failure of the first launch returns without the second.
 * Checked in this order: null tensors, null kv_lens, null cu_seqlens_q, the page geometry, B / Hkv, the table's alignment, cu_seqlens_q's
 * alignment, total_q / max_seqlen_q >= 1, is_causal, the grid's size, lse_sh, Hq / Hkv >= 2 (no GQA group to pack); then, refused by name,
 * SAGE_ATTR_KV_SPLIT, SAGE_ATTR_FP8_FOLDED_SCORES, SAGE_ATTR_FORCE_PERSISTENT and SAGE_ATTR_GQA_PACK (the entry packs on its own); a missing
 * q_start; then sage_kvpaged_attn's checks of head_dim, Hq % Hkv, dtypes, alignment and strides.
 */
SAGE_KVSTEP_API int sage_kvstep_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
                                     const float *k_scale, const float *v_scale, const int32_t *kv_lens, const int32_t *cu_seqlens_q,
                                     const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                     int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                                     int64_t q_sl, int64_t q_sh, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                     int64_t o_sl, int64_t o_sh, int64_t lse_sh,
                                     int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_KVSTEP_GFX950_H */
