/*
 * sage_kvlsplit_gfx950.h -- C ABI of the SPLIT step call on the paged quantised KV cache of libsage_gfx950.so (AMD MI355X, gfx950 / CDNA4):
 * include/sage_kvlist_gfx950.h's call with every DECODE sequence -- one of 1 .. 32 rows -- run as S key-range chunks, exactly.
 *
 * sage_kvlist_attn runs a decode sequence as Hkv * ceil(group / 4) serial chains over its whole context; a step of a handful of long contexts
 * leaves most of the device idle.  This entry splits those chains as include/sage_kvpsplit_gfx950.h splits a dense call's: a chunk is
 * T = ceil(ceil(capacity / 64) / S) whole 64-key tiles of the logical key axis (capacity = max_pages_per_seq * page_size), the same for every
 * sequence; pass 1 forms each chunk's row maxima, pass 2 runs the chunks seeded with the maxima in front of them and leaves FP32 partials, the
 * merge joins them.  For a decode sequence of n rows, o and lse are BIT FOR BIT what sage_kvpsplit_attn returns for that sample in a call of
 * Lq = n with the same S, SAGE_ATTR_GQA_PACK and the same offsets.  The sequences of more than 32 rows go through sage_kvlist_attn's chunk launch
 * as they are: their rows are bit for bit that entry's.  Rows no sequence owns are not written; a sequence without keys gives o = 0, lse = -inf.
 *
 * Launches on the caller's stream: plan (sage_kvlist_attn's, its workspace and lists unchanged: the decode list is sorted by context), pass 1,
 * pass 2 over units (decode-list rank, chunk, kv head) dealt to the XCDs round-robin, the merge, then the chunk launch if max_seqlen_q > 32 and
 * the list's bound is not 0.  Nothing is read on the host, nothing synchronises, nothing is allocated: the call captures into a HIP graph.  A
 * sequence shorter than the capacity has empty trailing chunks: each costs an early exit and one -inf word.
 *
 * The split workspace travels as in include/sage_gfx950.h's SAGE_ATTR_KV_SPLIT convention: SageLaunchAttr.flags carries SAGE_ATTR_KV_SPLIT and S in
 * bits 16-23, launch_ws / launch_ws_bytes the workspace, 128-byte aligned, sage_kvlsplit_ws_bytes(B, Hq, max_seqlen_q, D, S) bytes: chunk_max,
 * lse_part [B, Hkv, S, group, Lq_ws] and o_part [.., D], FP32, each segment rounded up to 128 bytes, with Lq_ws = min(max_seqlen_q, 32) rows per
 * (sequence, head) whatever the sequences' own row counts are.  Only the rows of decode sequences are written.
 *
 * Device rule as in include/sage_kvlist_gfx950.h: a bad prefix array or a workspace the plan never wrote gives wrong numbers or dropped work,
 * never an access outside the operands or the workspaces.
 *
 * Conventions as in include/sage_gfx950.h and include/sage_kvlist_gfx950.h (both unchanged, as are their ABI versions and every refusal of
 * SAGE_ATTR_KV_SPLIT by another entry): 0 or a negative code (-1: bad argument, -2: launch error), message in sage_last_error().  Argument errors
 * return -1 before anything touches a GPU.
 * Replaces in the reference: nothing (thu-ml/SageAttention has no KV cache).
 */
#ifndef SAGE_KVLSPLIT_GFX950_H
#define SAGE_KVLSPLIT_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_KVLSPLIT_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_KVLSPLIT_API __attribute__((visibility("default")))
#else
#define SAGE_KVLSPLIT_API
#endif

SAGE_KVLSPLIT_API int sage_kvlsplit_abi_version(void);

/*
 * bytes of the split workspace: 2 * r128(4 * B * Hq * S * Lq_ws) + r128(4 * B * Hq * S * Lq_ws * D) with Lq_ws = min(max_seqlen_q, 32) and r128
 * rounding up to 128; -1 for B, Hq or max_seqlen_q < 1, D not 64 / 128 or S outside [2, 255]
 */
SAGE_KVLSPLIT_API int64_t sage_kvlsplit_ws_bytes(int B, int Hq, int max_seqlen_q, int D, int S);

/*
 * sage_kvlist_attn's arguments, argument for argument, with its meanings.  SageLaunchAttr.grid_out receives pass 2's grid,
 * 8 * ceil(B * S * Hkv / 8) * ceil(Hq / Hkv / 4), plus the chunk launch's (sage_kvlist_plan_host's chunk_grid) when that launch is made.  A
 * failure of a launch returns without the launches behind it.
 * Checked in this order, every failure -1: sage_kvlist_attn's checks in its order under this entry's name (but SAGE_ATTR_KV_SPLIT is taken, not
 * refused); attr without SAGE_ATTR_KV_SPLIT; S outside [2, 255]; a non-zero SageLaunchAttr.window; the split workspace null, not 128-byte aligned
 * or shorter than sage_kvlsplit_ws_bytes(B, Hq, max_seqlen_q, D, S).
 */
SAGE_KVLSPLIT_API int sage_kvlsplit_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
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

#endif /* SAGE_KVLSPLIT_GFX950_H */
