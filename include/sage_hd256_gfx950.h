/*
 * sage_hd256_gfx950.h -- C ABI of the head_dim = 256 FP8-PV attention route of libsage_gfx950.so (AMD MI355X, gfx950 / CDNA4).
 *
 * Every entry of include/sage_gfx950.h takes head_dim 64 or 128.  The two calls here are the same arithmetic -- INT8 QK^T with per-thread
 * scale groups, the exact score form exp2(fma(s, c, -m)), e4m3 V with a per-channel scale at scale_max = 448, two-level FP32 accumulation
 * -- for head_dim = 256, on kernels of their own (csrc/sage_hd256_attn.hip, csrc/sage_hd256_prepass.hip).  A caller with
 * 128 < head_dim < 256 zero-pads to 256 and passes its own sm_scale.
 *
 *   sage_hd256_prepass   K: per-channel mean over the tokens (FP32 sum, rounded to the input dtype, subtracted in the input dtype; written
 *                        to k_mean in the input dtype, [B, Hkv, 256]); INT8 rows with the per-thread scale groups of 64-key tiles
 *                        (group (key % 8) / 2 of tile key / 64; scale = amax / 127 + 1e-7; x / scale, +-0.5, truncated) as the K IMAGE;
 *                        k_scale [B, Hkv, 4 * ntile].  V: per-channel amax over the tokens, v_scale = amax / 448 [B, Hkv, 256], e4m3 bytes
 *                        of v * (448 / amax) as the V IMAGE.  ntile = ceil(Lk / 64).  smooth_k = 0 leaves the mean out (k_mean is
 *                        written as zeros).  Two launches: per-chunk statistics into ws, then one workgroup per 64-key tile.
 *   sage_hd256_attn      o = softmax(q k^T sm_scale) v on the images; q is fp16 / bf16 and is quantised per thread group in the kernel's
 *                        prologue.  is_causal: row i sees keys j <= i (top-left).  lse (nullable) [B, Hq, Lq] fp32 in log2 units,
 *                        log2(l) + m of the scores q (k - mean)^T: the caller adds q . mean sm_scale as for the other entries.
 *
 * The images are private to this pair of calls: 16 KiB per (batch, kv head, 64-key tile), [B, Hkv, ntile, 16384] bytes each.
 *   K image   row r = key % 64 is 256 bytes; its 16-byte chunk c (channels 16 c .. 16 c + 15) stands at chunk c ^ (r & 15).
 *   V image   channel d is 64 bytes; byte p holds token 16 (p >> 3 & 3) + 8 (p >> 2 & 1) + 4 (p >> 5) + (p & 3) of the tile, and the
 *             16-byte chunk p >> 4 stands at chunk (p >> 4) ^ (d >> 2 & 3).
 *   Keys from Lk on in the last tile are zero bytes in both.
 *
 * q, k, v, o: element strides (batch, head, token), last dimension contiguous -- either tensor layout; 16-byte aligned, strides multiples
 * of 8.  Conventions as in include/sage_gfx950.h: caller-owned buffers, no allocation, no synchronisation, the caller's stream, graph
 * capturable.  0, or -1 (bad argument, nothing touched a GPU) / -2 (launch error) with the message in sage_last_error().  Argument checks in
 * this order: head_dim, dtype, an empty problem, Hq % Hkv, null pointers, alignment and strides, the workspace, the grid.
 * Replaces in the reference: nothing (thu-ml/SageAttention refuses head_dim > 128).
 */
#ifndef SAGE_HD256_GFX950_H
#define SAGE_HD256_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_HD256_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_HD256_API __attribute__((visibility("default")))
#else
#define SAGE_HD256_API
#endif

SAGE_HD256_API int sage_hd256_abi_version(void);

/* floats of the pre-pass workspace: 512 per (batch, kv head, 256-token chunk); -1 for an empty problem */
SAGE_HD256_API int64_t sage_hd256_ws_floats(int B, int Hkv, int Lk);

SAGE_HD256_API int sage_hd256_prepass(const void *k, const void *v, void *k_image, float *k_scale, void *k_mean, void *v_image, float *v_scale,
                                      float *ws, int64_t ws_floats, int B, int Hkv, int Lk, int head_dim,
                                      int64_t k_sb, int64_t k_sh, int64_t k_sl, int64_t v_sb, int64_t v_sh, int64_t v_sl,
                                      int smooth_k, int dtype, void *stream);

SAGE_HD256_API int sage_hd256_attn(const void *q, const void *k_image, const void *v_image, const float *k_scale, const float *v_scale,
                                   void *o, float *lse, int B, int Hq, int Hkv, int Lq, int Lk, int head_dim,
                                   int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                   int is_causal, float sm_scale, int dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_HD256_GFX950_H */
