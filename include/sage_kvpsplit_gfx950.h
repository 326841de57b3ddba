/*
 * sage_kvpsplit_gfx950.h -- C ABI of the EXACT SPLIT-KV call on the paged quantised KV cache of libsage_gfx950.so (AMD MI355X, gfx950 / CDNA4).
 *
 * include/sage_kvpaged_gfx950.h attends on a pool of pages behind a block table; sage_attn_fused_q_pv_f8_kvlens (include/sage_gfx950.h) with
 * SAGE_ATTR_KV_SPLIT runs a decode-shaped call as S chunks of the key range -- pass 1 (the chunk maxima), pass 2 (the chunks folded into the kv
 * heads, seeded with the maximum the unsplit call holds in front of each chunk, FP32 partials) and the merge -- so that few long sequences fill
 * the chip.  sage_kvpaged_attn refuses that flag.  This entry is the join: the same three launches with pass 1 and pass 2 looking their tiles
 * up in the table.
 *
 * Exactness: a chunk is T = ceil(ceil(Lk / 64) / S) whole 64-key tiles of the LOGICAL key axis, Lk = max_pages_per_seq * page_size; "which
 * tile" is a table lookup in both passes and the arithmetic is untouched.  sage_kvpsplit_attn returns -- output, LSE and every byte of the split
 * workspace -- what sage_attn_fused_q_pv_f8_kvlens with SAGE_ATTR_KV_SPLIT and the same S returns on a contiguous cache of the same content and
 * the same capacity.
 *
 * Device rules, as in include/sage_kvpaged_gfx950.h: a bad table gives wrong numbers, never an access outside the pool.  Chunk c of sample b reads
 * the table entries of its own tiles c * T .. c * T + T - 1 that lie in front of ceil(len_b / 64) and no others; a chunk from len_b on reads none,
 * a chunk that lies wholly behind the diagonal of the call's 128-row query block reads none, a sample without keys reads none.  A chunk need not
 * start on a page boundary.
 * Every id read is clamped to [0, num_pages - 1] on the scalar unit before it forms an address.
 *
 * Conventions as in include/sage_gfx950.h (SAGE_ABI_VERSION, SAGE_KVCACHE_ABI_VERSION, SAGE_KVPAGED_ABI_VERSION and SAGE_KVFORK_ABI_VERSION are
 * untouched): caller-owned buffers, no state, no allocation, no host read of any tensor, no synchronisation, grids from the shapes alone -- the
 * call captures into a HIP graph and a replay follows the table's and the lengths' contents.  Strides in ELEMENTS; 0 or a negative code (-1: bad
 * argument, -2: launch error), message in sage_last_error().  Argument errors return -1 before anything touches a GPU.
 * Replaces in the reference: nothing (thu-ml/SageAttention has no KV cache and does not split the key range).
 */
#ifndef SAGE_KVPSPLIT_GFX950_H
#define SAGE_KVPSPLIT_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_KVPSPLIT_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_KVPSPLIT_API __attribute__((visibility("default")))
#else
#define SAGE_KVPSPLIT_API
#endif

SAGE_KVPSPLIT_API int sage_kvpsplit_abi_version(void);

/*
 * sage_kvpaged_attn's argument list, argument for argument.  `attr` is required and carries SAGE_ATTR_KV_SPLIT, the chunk count S in flags bits
 * 16-23 and the split workspace in launch_ws / launch_ws_bytes: the convention, alignment (128 bytes), segment layout (chunk_max, lse_part
 * [B, Hkv, S, group, Lq] and o_part [.., D], fp32, each segment rounded up to 128 bytes) and size of sage_attn_fused_q_pv_f8_kvlens.  q_start,
 * SAGE_ATTR_GQA_PACK and grid_out mean what they mean there; grid_out reports pass 2's grid.
 * Argument errors, each named "sage_kvpsplit_attn": the page geometry and the table's alignment (as sage_kvpaged_attn), attr without
 * SAGE_ATTR_KV_SPLIT, S outside [2, 255], Lq > 128, a non-zero window, SAGE_ATTR_FP8_FOLDED_SCORES, SAGE_ATTR_FORCE_PERSISTENT, a null,
 * misaligned or short workspace; then what sage_attn_fused_q_pv_f8_kvlens checks of its tensors.
 */
SAGE_KVPSPLIT_API int sage_kvpsplit_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
                                         const float *k_scale, const float *v_scale, const int32_t *kv_lens,
                                         const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                         int B, int Hq, int Hkv, int Lq, int D,
                                         int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                         int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                         int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_KVPSPLIT_GFX950_H */
