/*
 * sage_mlacache_gfx950.h -- C ABI of the APPENDABLE quantised latent of the absorbed MLA decode route of libsage_gfx950.so (AMD MI355X, gfx950 /
 * CDNA4): rows are added in place, and exactly, to the operands that sage_mla_attn and sage_mlasplit_attn take (include/sage_mla_gfx950.h,
 * include/sage_mlasplit_gfx950.h), so a decode step costs two small launches instead of the pre-pass over the whole latent.
 *
 * The cache is those operands with the tile count of its capacity -- k_image [B, ntile, 36864], v_image [B, ntile, 32768], k_scale [B, 4 ntile],
 * v_scale [B, 512], ntile = ceil(capacity / 64) -- and, beside them, k_mean [B, 576] (input dtype) and v_amax [B, 512] (fp32), the FROZEN
 * statistics; lens [B] int32, the rows each sample holds; and tail [B, 64, 576] (input dtype), the raw rows of each sample's open tile.  Attention
 * is sage_mla_attn(..., kv_lens = lens, Lk = capacity, ...): no attention kernel knows about the cache.
 *
 * Why appending is exact (csrc/sage_mla_cache.hip).  Softmax does not change when one vector is subtracted from every key, so a
 * frozen k_mean is as exact as a running one.  The per-thread K scale group (key % 8) / 2 is local to a 64-key tile and its abs-max runs over the
 * valid rows only, so new rows change the tile that holds row len - 1 (the open tile) and no other; that tile is re-quantised from its raw rows
 * each time it grows, which is what the tail is for.  With v_amax frozen a token's e4m3 byte depends on that token alone: v * (448 / v_amax), 0
 * for a channel whose v_amax is 0, saturated at +-448 beyond the range.  Seeded with the statistics of its final content a cache holds, byte for
 * byte, what sage_mla_prepass makes of that content, whatever the schedule of appends.
 *
 *   sage_mlacache_stats    the statistics of a prompt kv [B, Lk, 576] behind (batch, token) element strides, kv_lens (nullable) int32 [B] on the
 *                          device: the pre-pass's statistics launch and its fold (ws: sage_mla_ws_floats(B, Lk) floats), k_mean [B, 576] in the
 *                          input dtype (zeros with smooth_k = 0 and for a sample of no rows) and v_amax [B, 512], the FP32 maxima themselves
 *                          (v_scale = amax / 448 does not give them back bit for bit).  Two launches.
 *   sage_mlacache_append   kv_new [B, T, 576] behind (batch, token) element strides.  Sample b takes the first n = min(max(new_lens[b], 0), T)
 *                          rows (new_lens nullable: T), cut to capacity - lens[b]: rows that do not fit are dropped on the device, and rows at or
 *                          behind n are never read.  Launch 1, grid (ceil((63 + T) / 64), B): workgroup (j, b) re-forms tile lens[b] / 64 + j if
 *                          it receives a row -- K image tile, its four k_scale slots, V image tile with zeros behind the last token -- from the
 *                          tail (rows in front of lens[b]) and kv_new; j = 0 also writes v_scale = v_amax / 448.  Launch 2, grid (B): the rows
 *                          of the new open tile that came from kv_new go to the tail, then lens[b] advances.  No two workgroups of launch 1 write
 *                          the same byte; launch 2 alone writes tail and lens.
 *
 * Conventions as in include/sage_gfx950.h: caller-owned buffers, no allocation, no synchronisation with the host, the caller's stream, graph
 * capturable (the grids are sized from B, T, capacity and Lk on the host; a replay follows the contents of kv_new, new_lens and lens).  kv and
 * kv_new: 16-byte aligned, strides multiples of 8 elements, rows at least 576 apart.  0, or -1 (bad argument, nothing touched a GPU) / -2 (launch
 * error) with the message in sage_last_error().  Argument checks in this order -- sage_mlacache_stats: dtype, an empty problem, null pointers
 * (only kv_lens may be null), alignment and strides of kv, alignment of the other buffers, the workspace, the grid; sage_mlacache_append: dtype,
 * an empty problem (B, T, capacity), null pointers (only new_lens may be null), alignment and strides of kv_new, alignment of the other buffers,
 * the grid.
 * Replaces in the reference: nothing (thu-ml/SageAttention has no cache and no width above 128).
 */
#ifndef SAGE_MLACACHE_GFX950_H
#define SAGE_MLACACHE_GFX950_H

#include <stdint.h>

#include "sage_mla_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_MLACACHE_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_MLACACHE_API __attribute__((visibility("default")))
#else
#define SAGE_MLACACHE_API
#endif

SAGE_MLACACHE_API int sage_mlacache_abi_version(void);

SAGE_MLACACHE_API int sage_mlacache_stats(const void *kv, const int32_t *kv_lens, void *k_mean, float *v_amax, float *ws, int64_t ws_floats,
                                          int B, int Lk, int64_t kv_sb, int64_t kv_sl, int smooth_k, int dtype, void *stream);

SAGE_MLACACHE_API int sage_mlacache_append(const void *kv_new, const int32_t *new_lens, int32_t *lens, void *tail, const void *k_mean,
                                           const float *v_amax, void *k_image, float *k_scale, void *v_image, float *v_scale, int B, int T,
                                           int capacity, int64_t kvn_sb, int64_t kvn_sl, int smooth_k, int dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_MLACACHE_GFX950_H */
