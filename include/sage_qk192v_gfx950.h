/*
 * sage_qk192v_gfx950.h -- C ABI of the PACKED (variable-length) form of the FP8-PV attention route for 192-wide Q / K rows against 128-wide V
 * rows of libsage_gfx950.so (AMD MI355X, gfx950 / CDNA4): the multi-head-latent-attention prefill as serving stacks call it -- q
 * [total_q, Hq, 192], k [total_k, Hkv, 192], v [total_k, Hkv, 128] behind the prefix arrays cu_seqlens_q / cu_seqlens_k (int32 [nseq + 1] on
 * the device), causal aligned top-left or bottom-right.  include/sage_qk192_gfx950.h is the dense form; its arithmetic and image formats are
 * this header's, and every sequence of a packed call is the dense call on its own slice.
 *
 *   sage_qk192v_ws_bytes   bytes of the workspace the two calls share: the plan (int32: header, counts, tile and chunk prefixes, the work
 *                          list, tile -> sequence and chunk -> sequence maps) and the statistics (320 floats per kv head and 256-token chunk).
 *                          Sized on the host from nseq, Hkv, total_q, total_k; -1 for an empty problem.
 *   sage_qk192v_prepass    four launches: the plan (sequence s owns 64-key tiles cu_kt[s] .. cu_kt[s + 1] - 1, counted from ITS first key: a
 *                          tile never spans two sequences; the (sequence, 128-row block) work list, heaviest first under `mask`), the
 *                          maps, the statistics (one workgroup per 256-token chunk of a sequence and kv head) and the quantiser (one per tile).
 *                          K mean per (sequence, kv head) over that sequence's keys, k_mean [nseq, Hkv, 192] in the input dtype (zeros for a
 *                          sequence without keys and when smooth_k = 0); k_scale [Hkv, 4 * tiles_cap]; v_scale [nseq, Hkv, 128]; the K image
 *                          [Hkv, tiles_cap, 12288] and the V image [Hkv, tiles_cap, 8192] in the dense header's tile formats, the keys of a
 *                          sequence's last tile from its length on zero bytes.  tiles_cap = ceil(total_k / 64) + nseq.
 *   sage_qk192v_attn       o [total_q, Hq, 128] = softmax(q k^T sm_scale) v per sequence.  mask: 0 none, 1 causal top-left (row i of a
 *                          sequence sees its keys j <= i), 2 causal bottom-right (j <= i + Lk_s - Lq_s).  A row that sees no key -- in front
 *                          of key 0, or of a sequence without keys -- gets o = +0 and lse = -inf.  lse (nullable) [Hq, total_q] fp32 in log2
 *                          units of the scores q (k - mean)^T: the caller adds q . mean_s sm_scale.  One workgroup per (work item, query head)
 *                          of a grid sized for ceil(total_q / 128) + nseq items; the true count stays on the device.
 *
 * `mask` of the pre-pass only orders the work list; pass the attention call's.  A cu_seqlens that disagrees with total_q / total_k (a last
 * prefix beyond the rows, not monotonic) drops work -- the result is then as undefined as the input -- and never reads or writes outside
 * the caller's buffers: every count and row derived from it on the device is clamped to the sizes given here.
 *
 * q, k, v, o: element strides (token, head), last dimension contiguous; 16-byte aligned, strides multiples of 8, non-negative; the head stride
 * of q and k at least 192, of v and o at least 128.  Conventions as in include/sage_gfx950.h: caller-owned buffers, no allocation, no
 * synchronisation, the caller's stream, graph capturable.  0, or -1 (bad argument, nothing touched a GPU) / -2 (launch error) with the message
 * in sage_last_error().  Argument checks in this order: head_dim_qk and head_dim_v, dtype, mask, an empty problem, nseq, Hq % Hkv, null
 * pointers, alignment and strides of the tensors, alignment of the other buffers, the workspace, the grid.
 * Replaces in the reference: nothing (thu-ml/SageAttention takes one head_dim for q, k and v, and none above 128).
 */
#ifndef SAGE_QK192V_GFX950_H
#define SAGE_QK192V_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_QK192V_ABI_VERSION 1

#define SAGE_QK192V_MASK_NONE 0
#define SAGE_QK192V_MASK_TOP_LEFT 1
#define SAGE_QK192V_MASK_BOTTOM_RIGHT 2

#if defined(__GNUC__)
#define SAGE_QK192V_API __attribute__((visibility("default")))
#else
#define SAGE_QK192V_API
#endif

SAGE_QK192V_API int sage_qk192v_abi_version(void);

SAGE_QK192V_API int64_t sage_qk192v_ws_bytes(int nseq, int Hkv, int total_q, int total_k);

SAGE_QK192V_API int sage_qk192v_prepass(const void *k, const void *v, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k,
                                        void *k_image, float *k_scale, void *k_mean, void *v_image, float *v_scale, void *ws, int64_t ws_bytes,
                                        int nseq, int total_q, int total_k, int Hq, int Hkv, int head_dim_qk, int head_dim_v,
                                        int64_t k_sl, int64_t k_sh, int64_t v_sl, int64_t v_sh, int mask, int smooth_k, int dtype, void *stream);

SAGE_QK192V_API int sage_qk192v_attn(const void *q, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, const void *k_image,
                                     const void *v_image, const float *k_scale, const float *v_scale, const void *ws, int64_t ws_bytes,
                                     void *o, float *lse, int nseq, int total_q, int total_k, int Hq, int Hkv, int head_dim_qk, int head_dim_v,
                                     int64_t q_sl, int64_t q_sh, int64_t o_sl, int64_t o_sh, int mask, float sm_scale, int dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_QK192V_GFX950_H */
