/*
 * sage_kvcache_gfx950.h -- C ABI of the appendable quantised KV cache of libsage_gfx950.so (AMD MI355X, gfx950 / CDNA4).
 *
 * A decode step adds one token to a context of thousands, and the K / V pre-pass of include/sage_gfx950.h (K mean, INT8 K, FP8 V image) runs
 * over the whole context each time.  The cache keeps exactly the operands that sage_attn_fused_q_pv_f8_kvlens takes -- INT8 K rows with
 * per-thread scales of 64-key blocks, the FP8 V tile image, the V scales, the lengths -- and this entry appends rows to them in place.  It is
 * attended through that entry with Lk = capacity and kv_lens = lens; no attention kernel knows about the cache.
 *
 * The statistics are FROZEN when the cache is seeded: `k_mean` (softmax is invariant under a constant vector subtracted from every key, so any
 * mean is exact; smoothing is about INT8 range only) and `v_amax` (the per-channel abs-max the FP8 conversion divides by; e4m3 is floating
 * point, so head-room on it costs no relative precision above the subnormal range, and values beyond it saturate at +-448 as they do in the
 * pre-pass).  With both fixed, an appended row changes no byte outside the one 64-key block it lands in: that block (the OPEN block, the one
 * that holds row len - 1 or starts at row len) is re-formed from its raw rows, which the cache keeps in `k_tail` / `v_tail`.  The bytes are those
 * of sage_quant_qk_int8_kvlens(k, k_mean, lens) and of sage_prep_v_fp8_kvlens's image for a V whose per-channel abs-max is `v_amax`: same device
 * arithmetic, shared in csrc/sage_kv_block.h.
 *
 * It shares the conventions of include/sage_gfx950.h (which this header does not change; SAGE_ABI_VERSION is untouched): the caller owns every
 * buffer, the library keeps no state and allocates nothing, work is enqueued on `stream` without synchronising, strides are in ELEMENTS, every
 * function returns 0 or a negative code (-1: bad argument, -2: launch error) and sage_last_error() of include/sage_gfx950.h holds the message.
 * Replaces in the reference: nothing (thu-ml/SageAttention has no KV cache; its callers quantise the whole K / V per call, core.py:636-826).
 */
#ifndef SAGE_KVCACHE_GFX950_H
#define SAGE_KVCACHE_GFX950_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_KVCACHE_ABI_VERSION 1

#if defined(__GNUC__)
#define SAGE_KVCACHE_API __attribute__((visibility("default")))
#else
#define SAGE_KVCACHE_API
#endif

SAGE_KVCACHE_API int sage_kvcache_abi_version(void);

/*
 * Append up to T rows per sample to a cache of B samples x Hkv kv-heads x `capacity` rows (a positive multiple of 64), head_dim 64 / 128.
 *
 * Cache state, device memory, contiguous, 16-byte aligned, shapes fixed at allocation:
 *  k_int8   int8  [B, Hkv, capacity, head_dim]       rows < lens[b] valid; the open block's rows are rewritten when it grows
 *  k_scale  fp32  [B, Hkv, capacity / 64 * 4]        per-thread scale groups, four per 64-key block; all four slots of a block that receives
 *                                                    a row are written (groups without a valid row: 1e-7, as the pre-pass writes them)
 *  v_image  uint8 [B, Hkv, capacity / 64, head_dim, 64]  the FP8 tile image of sage_prep_v_fp8 (csrc/sage_prep_v.hip), a whole tile per block
 *                                                    that receives a row: positions behind the last valid token are zero
 *  v_scale  fp32  [B, Hkv, head_dim]                 OUT: v_amax / 448 by the pre-pass's expression, written by every call (same bytes each time)
 *  v_amax   fp32  [B, Hkv, head_dim]                 IN, frozen: the per-channel abs-max the conversion uses (0: the channel's image is zero)
 *  k_mean   dtype [B, Hkv, head_dim]                 IN, frozen, NULLABLE (no smoothing): subtracted from a key, rounded to `dtype`, first
 *  k_tail   dtype [B, Hkv, 64, head_dim]             the raw rows of the open block at their position in the block; rows at or behind
 *  v_tail   dtype [B, Hkv, 64, head_dim]             lens[b] % 64 are never read
 *  lens     int32 [B]                                IN / OUT: rows each sample holds, clamped to [0, capacity] on the device when read
 * New rows:
 *  k_new, v_new  dtype [B, Hkv, T, head_dim] with element strides (batch, head, row; multiples of 8, innermost stride 1): HND and NHD views
 *                both fit.  Rows at or behind the sample's count are never read (they may hold anything).
 *  new_lens      int32 [B], NULLABLE (null: T rows for every sample): rows to take from sample b, clamped on the device to [0, T] and then
 *                to capacity - lens[b]: what does not fit is dropped and nothing is written past a buffer.
 *
 * Two launches on `stream`, grids from the shapes alone, no host read of any tensor, no synchronisation, no allocation: the call captures
 * into a HIP graph and a replay follows the tensors' contents.  Launch 1 (ceil((63 + T) / 64) x Hkv x B workgroups) re-forms every block that
 * receives a row, reading `lens` and the tails; launch 2 (B workgroups) copies the new open block's new rows into the tails and then stores
 * lens[b] -- workgroup b alone touches sample b's tails and length, and stream order puts it behind launch 1's reads.
 * Never read: k_int8, k_scale, v_image, v_scale.  Argument errors (a null pointer where one is required, head_dim, T < 1, capacity, alignment,
 * strides, dtype) return -1 before anything touches a GPU.
 */
SAGE_KVCACHE_API int sage_kvcache_append(int8_t *k_int8, float *k_scale, void *v_image, float *v_scale, const float *v_amax, const void *k_mean,
                                         void *k_tail, void *v_tail, int32_t *lens,
                                         const void *k_new, const void *v_new, const int32_t *new_lens,
                                         int B, int Hkv, int capacity, int T, int head_dim,
                                         int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                         int64_t v_sb, int64_t v_sh, int64_t v_sl,
                                         int dtype, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SAGE_KVCACHE_GFX950_H */
