/*
 * sage_mla_gfx950.h -- C ABI of the FP8-PV attention route for the ABSORBED multi-head-latent-attention decode shape of libsage_gfx950.so (AMD
 * MI355X, gfx950 / CDNA4): every query head reads one shared latent row of 576 channels per token (512 compressed + 64 rope), and V is the first
 * 512 channels of that same row.
 *
 * include/sage_gfx950.h stops at head_dim 128, include/sage_hd256_gfx950.h at 256, include/sage_qk192_gfx950.h at 192 / 128, and none of them
 * lets V be a slice of K.  The calls here are the same arithmetic -- K smoothed by its per-channel mean, INT8 QK^T with the per-thread scale
 * groups of K and ONE scale per query row, the exact score form exp2(fma(s, c, -m)), e4m3 V with a per-channel scale at scale_max = 448,
 * two-level FP32 accumulation -- for width_qk = 576 and width_v = 512, on kernels of their own (csrc/sage_mla_attn.hip,
 * csrc/sage_mla_prepass.hip).
 *
 *   sage_mla_prepass   kv [B, Lk, 576] fp16 / bf16 behind (batch, token) element strides.  kv_lens (nullable: every sample has Lk rows) is
 *                      int32 [B] ON THE DEVICE; sample b has min(max(kv_lens[b], 0), Lk) valid rows and no row from there on is read.
 *                      K: per-channel mean over the valid rows (FP32 sum, rounded to the input dtype, subtracted in the input dtype; k_mean
 *                      [B, 576] in the input dtype, zeros with smooth_k = 0); INT8 rows with the per-thread scale groups of 64-key tiles
 *                      (group (key % 8) / 2 of tile key / 64; scale = amax / 127 + 1e-7; x / scale, +-0.5, truncated) as the K IMAGE; k_scale
 *                      [B, 4 * ntile].  V = kv[..., :512]: per-channel amax over the valid rows, v_scale = amax / 448 [B, 512], e4m3 bytes of
 *                      v * (448 / amax) as the V IMAGE.  ntile = ceil(Lk / 64); tiles wholly behind a sample's length are left unwritten and
 *                      are never read.  Three launches: per-chunk statistics into ws, their fold per sample, one workgroup per 64-key tile.
 *   sage_mla_attn      q [B, Lq, Hq, 576] behind (batch, position, head) element strides, quantised in the kernel's prologue; o
 *                      [B, Lq, Hq, 512] contiguous.  The mask is the decode one: position i of sample b sees key j iff
 *                      j <= kv_lens[b] - Lq + i.  A position in front of key 0 gets o = +0 and lse = -inf.  lse (nullable) [B, Hq, Lq] fp32 in
 *                      log2 units, log2(l) + m of the scores q (k - mean)^T: the caller adds q . mean sm_scale as for the other entries.
 *                      The kernel takes 136 KiB of LDS per workgroup; a device that offers less is refused with -1.
 *
 * The images are private to this pair of calls.
 *   K image   [B, ntile, 36864] bytes.  A tile is nine panels of 4096 bytes; panel P holds channels 64 P .. 64 P + 63 of the tile's 64 keys.
 *             Channel x of key r is byte 4096 (x >> 6) + 64 r + 16 ((x >> 4 & 3) ^ (r >> 2 & 3)) + (x & 15).
 *   V image   [B, ntile, 32768] bytes.  Channel d is 64 bytes; byte p holds token 16 (p >> 3 & 3) + 8 (p >> 2 & 1) + 4 (p >> 5) + (p & 3) of the
 *             tile, at byte 64 d + 16 ((p >> 4) ^ (d >> 2 & 3)) + (p & 15).
 *   Keys from a sample's length on in its last tile are zero bytes in both.
 *
 * Conventions as in include/sage_gfx950.h: caller-owned buffers, no allocation, no synchronisation with the host, the caller's stream, graph
 * capturable (grids are sized from B, Lk and Lq * Hq on the host).  kv and q: 16-byte aligned, strides multiples of 8 elements, rows at least
 * 576 apart.  0, or -1 (bad argument, nothing touched a GPU) / -2 (launch error) with the message in sage_last_error().  Argument checks in
 * this order: the widths, dtype, an empty problem, null pointers, alignment and strides of the tensors, alignment of the other buffers, the
 * workspace, the grid, the device's LDS.
 * Replaces in the reference: nothing (thu-ml/SageAttention takes one head_dim for q, k and v, and none above 128).
 */
#ifndef SAGE_MLA_GFX950_H
#define SAGE_MLA_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_MLA_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_MLA_API __attribute__((visibility("default")))
#else
#define SAGE_MLA_API
#endif

SAGE_MLA_API int sage_mla_abi_version(void);

/* floats of the pre-pass workspace: 1088 per (sample, 256-token chunk) and 512 more per sample; -1 for an empty problem */
SAGE_MLA_API int64_t sage_mla_ws_floats(int B, int Lk);

SAGE_MLA_API int sage_mla_prepass(const void *kv, const int32_t *kv_lens, void *k_image, float *k_scale, void *k_mean, void *v_image,
                                  float *v_scale, float *ws, int64_t ws_floats, int B, int Lk, int width_qk, int width_v,
                                  int64_t kv_sb, int64_t kv_sl, int smooth_k, int dtype, void *stream);

SAGE_MLA_API int sage_mla_attn(const void *q, const void *k_image, const void *v_image, const float *k_scale, const float *v_scale,
                               const int32_t *kv_lens, void *o, float *lse, int B, int Lq, int Hq, int Lk, int width_qk, int width_v,
                               int64_t q_sb, int64_t q_sl, int64_t q_sh, float sm_scale, int dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_MLA_GFX950_H */
