/*
 * sage_mlasplit_gfx950.h -- C ABI of the EXACT split of the key range for the absorbed MLA decode route of libsage_gfx950.so (AMD MI355X,
 * gfx950 / CDNA4): sage_mla_attn (include/sage_mla_gfx950.h) with every work item run as S key-range chunks on S times as many workgroups.
 *
 * sage_mla_attn gives one workgroup a sample's whole latent, so a call takes the time of one workgroup's serial chain however few of the
 * chip's CUs it fills.  sage_mlasplit_attn computes what sage_mla_attn computes -- every e4m3 P is the P of that call, bit for bit; only the
 * FP32 summation order of O and l differs -- in three launches on the caller's stream (csrc/sage_mla_split.hip):
 *
 *   chunking   T = ceil(ceil(Lk / 64) / S) tiles per chunk, from the shapes alone.  Chunk c of sample b holds the keys
 *              [64 T c, 64 T (c + 1)) below the sample's length min(max(kv_lens[b], 0), Lk).  The mask j <= kv_lens[b] - Lq + i stays in global
 *              key coordinates.  A chunk that holds no key any row of its work item sees requests no tile and no scale in either pass.
 *   pass 1     chunk_max [B, S, rows]: for every (sample, chunk, row) the running row maximum the attention loop forms over that chunk's keys
 *              alone, -inf where the row sees none of them.
 *   pass 2     the attention loop of sage_mla_attn on one chunk, its running maximum started from max over c' < c of chunk_max[b, c', row]:
 *              lse_part [B, S, rows] = log2(l) + m (-inf at l = 0) and o_part [B, S, rows, 512] = O (1 / l) v_scale in FP32.  A work item
 *              whose chunk shows no key to any of its rows writes lse_part = -inf and leaves o_part unwritten.
 *   merge      with M = max_c lse_part and w_c = exp2(lse_part_c - M): o = sum_c w_c o_part_c / sum_c w_c, cast once, and
 *              lse = M + log2(sum_c w_c) in log2 units.  A chunk at -inf is skipped without reading its o_part; all chunks at -inf give
 *              o = +0, lse = -inf.
 *
 * Workspace: caller-owned, 128-byte aligned, three FP32 segments in this order, each rounded up to a multiple of 128 bytes -- chunk_max, lse_part,
 * o_part -- with rows = Lq * Hq; sage_mlasplit_ws_bytes gives the total.  Every element of chunk_max and lse_part is written by every call.
 *
 * The arguments are sage_mla_attn's, followed by num_splits, ws, ws_bytes; o, lse and the images are what that call takes.  Conventions as in
 * include/sage_gfx950.h: no allocation, no synchronisation with the host, the caller's stream, graph capturable (the grids are sized from B,
 * Lq * Hq and num_splits on the host).  0, or -1 (bad argument, nothing touched a GPU) / -2 (launch error) with the message in
 * sage_last_error().  Argument checks in this order: everything sage_mla_attn refuses in front of its LDS check, in its order; num_splits
 * outside [2, 255]; a null, misaligned or short workspace; a grid of 2^31 or more; the device's LDS (pass 2 takes 136 KiB per workgroup, pass 1
 * 72 KiB).
 * Replaces in the reference: nothing.
 */
#ifndef SAGE_MLASPLIT_GFX950_H
#define SAGE_MLASPLIT_GFX950_H

#include <stdint.h>

#include "sage_mla_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_MLASPLIT_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_MLASPLIT_API __attribute__((visibility("default")))
#else
#define SAGE_MLASPLIT_API
#endif

SAGE_MLASPLIT_API int sage_mlasplit_abi_version(void);

/* bytes of the workspace: 2 * round128(4 B S rows) + round128(2048 B S rows), rows = Lq * Hq; -1 for an empty problem or S outside [2, 255] */
SAGE_MLASPLIT_API int64_t sage_mlasplit_ws_bytes(int B, int Lq, int Hq, int num_splits);

SAGE_MLASPLIT_API int sage_mlasplit_attn(const void *q, const void *k_image, const void *v_image, const float *k_scale, const float *v_scale,
                                         const int32_t *kv_lens, void *o, float *lse, int B, int Lq, int Hq, int Lk, int width_qk, int width_v,
                                         int64_t q_sb, int64_t q_sl, int64_t q_sh, float sm_scale, int dtype, void *stream, int num_splits,
                                         void *ws, int64_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_MLASPLIT_GFX950_H */
