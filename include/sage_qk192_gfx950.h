/*
 * sage_qk192_gfx950.h -- C ABI of the FP8-PV attention route for 192-wide Q / K rows against 128-wide V rows of libsage_gfx950.so (AMD
 * MI355X, gfx950 / CDNA4): the multi-head-latent-attention prefill shape (128 "nope" + 64 rope channels of Q and K, 128 of V).
 *
 * Every entry of include/sage_gfx950.h takes one head_dim of 64 or 128 for q, k and v; include/sage_hd256_gfx950.h one of 256.  The two calls
 * here are the same arithmetic -- INT8 QK^T with per-thread scale groups, the exact score form exp2(fma(s, c, -m)), e4m3 V with a per-channel
 * scale at scale_max = 448, two-level FP32 accumulation -- for head_dim_qk = 192 and head_dim_v = 128, on kernels of their own
 * (csrc/sage_qk192_attn.hip, csrc/sage_qk192_prepass.hip).  A caller with 128 < head_dim_qk < 192 or head_dim_v < 128
 * zero-pads and passes its own sm_scale.
 *
 *   sage_qk192_prepass   K: per-channel mean over the tokens (FP32 sum, rounded to the input dtype, subtracted in the input dtype; written
 *                        to k_mean in the input dtype, [B, Hkv, 192]); INT8 rows with the per-thread scale groups of 64-key tiles
 *                        (group (key % 8) / 2 of tile key / 64; scale = amax / 127 + 1e-7; x / scale, +-0.5, truncated) as the K IMAGE;
 *                        k_scale [B, Hkv, 4 * ntile].  V: per-channel amax over the tokens, v_scale = amax / 448 [B, Hkv, 128], e4m3 bytes
 *                        of v * (448 / amax) as the V IMAGE.  ntile = ceil(Lk / 64).  smooth_k = 0 leaves the mean out (k_mean is
 *                        written as zeros).  Two launches: per-chunk statistics into ws, then one workgroup per 64-key tile.
 *   sage_qk192_attn      o = softmax(q k^T sm_scale) v on the images; q (rows of 192) is fp16 / bf16 and is quantised per thread group in
 *                        the kernel's prologue; o has rows of 128.  is_causal: row i sees keys j <= i (top-left).  lse (nullable)
 *                        [B, Hq, Lq] fp32 in log2 units, log2(l) + m of the scores q (k - mean)^T: the caller adds q . mean sm_scale as
 *                        for the other entries.
 *
 * The images are private to this pair of calls.
 *   K image   [B, Hkv, ntile, 12288] bytes.  A tile is three panels of 4096 bytes; panel P holds channels 64 P .. 64 P + 63 of the tile's
 *             64 keys.  Inside a panel row r = key % 64 is 64 bytes, and its 16-byte chunk c (channels 64 P + 16 c .. + 15) stands at chunk
 *             c ^ (r >> 2 & 3): channel x of key r is byte 4096 (x >> 6) + 64 r + 16 ((x >> 4 & 3) ^ (r >> 2 & 3)) + (x & 15).
 *   V image   [B, Hkv, ntile, 8192] bytes.  Channel d is 64 bytes; byte p holds token 16 (p >> 3 & 3) + 8 (p >> 2 & 1) + 4 (p >> 5) + (p & 3)
 *             of the tile, and the 16-byte chunk p >> 4 stands at chunk (p >> 4) ^ (d >> 2 & 3): byte 64 d + 16 ((p >> 4) ^ (d >> 2 & 3)) + (p & 15).
 *   Keys from Lk on in the last tile are zero bytes in both.
 *
 * q, k, v, o: element strides (batch, head, token), last dimension contiguous -- either tensor layout; 16-byte aligned, strides multiples
 * of 8; the token stride of q and k is at least 192, of v and o at least 128.  Conventions as in include/sage_gfx950.h: caller-owned
 * buffers, no allocation, no synchronisation, the caller's stream, graph capturable.  0, or -1 (bad argument, nothing touched a GPU) / -2
 * (launch error) with the message in sage_last_error().  Argument checks in this order: head_dim_qk and head_dim_v, dtype, an empty problem,
 * Hq % Hkv, null pointers, alignment and strides of the tensors, alignment of the other buffers, the workspace, the grid.
 * Replaces in the reference: nothing (thu-ml/SageAttention takes one head_dim for q, k and v, and none above 128).
 */
#ifndef SAGE_QK192_GFX950_H
#define SAGE_QK192_GFX950_H

#include <stdint.h>

#include "sage_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_QK192_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_QK192_API __attribute__((visibility("default")))
#else
#define SAGE_QK192_API
#endif

SAGE_QK192_API int sage_qk192_abi_version(void);

/* floats of the pre-pass workspace: 320 per (batch, kv head, 256-token chunk); -1 for an empty problem */
SAGE_QK192_API int64_t sage_qk192_ws_floats(int B, int Hkv, int Lk);

SAGE_QK192_API int sage_qk192_prepass(const void *k, const void *v, void *k_image, float *k_scale, void *k_mean, void *v_image, float *v_scale,
                                      float *ws, int64_t ws_floats, int B, int Hkv, int Lk, int head_dim_qk, int head_dim_v,
                                      int64_t k_sb, int64_t k_sh, int64_t k_sl, int64_t v_sb, int64_t v_sh, int64_t v_sl,
                                      int smooth_k, int dtype, void *stream);

SAGE_QK192_API int sage_qk192_attn(const void *q, const void *k_image, const void *v_image, const float *k_scale, const float *v_scale,
                                   void *o, float *lse, int B, int Hq, int Hkv, int Lq, int Lk, int head_dim_qk, int head_dim_v,
                                   int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                   int is_causal, float sm_scale, int dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_QK192_GFX950_H */
