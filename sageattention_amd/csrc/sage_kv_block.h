// sage_kv_block.h -- the per-block arithmetic of the K quantiser (sage_quant.hip) and of the FP8 V image (sage_prep_v.hip), shared with the
// appendable cache (sage_kv_cache.hip), which re-forms one 64-key block with the same operations and therefore the same bits.
#pragma once
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_quant_math.h"

namespace sage {

// ---- INT8 rows -------------------------------------------------------------------------------------------------------
// One 16-element chunk of a row: the raw fp16 / bf16 words (and the mean's, with has_mean) -> fp32 values in v, their abs-max returned.
template <int DT>
__device__ __forceinline__ float quant_load16(const v4u (&raw)[2], const v4u (&mraw)[2], bool has_mean, int style, float pre_scale, float (&v)[16])
{
    float amax = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const unsigned w = raw[j >> 3][(j & 7) >> 1];
        float f = ld16<DT>((uint16_t)((j & 1) ? (w >> 16) : (w & 0xffffu)));
        if (has_mean) {
            const unsigned mw = mraw[j >> 3][(j & 7) >> 1];
            f = f - ld16<DT>((uint16_t)((j & 1) ? (mw >> 16) : (mw & 0xffffu)));
            // torch's `k - km` rounds to the input dtype (quant_per_block.py:53-54);
            // the CUDA quantiser keeps the fp32 difference (fused.cu:131-137)
            if (style != QS_CUDA) f = ld16<DT>(st16<DT>(f));
        }
        f *= pre_scale;
        v[j] = f;
        amax = fmaxf(amax, fabsf(f));
    }
    return amax;
}

// The 16 INT8 values of such a chunk, packed, from the abs-max `am` of its scale group.
__device__ __forceinline__ v4u quant_pack16(const float (&v)[16], float am, int style)
{
    int q[16];
    if (style == QS_CUDA) {
        const float inv = 127.0f / am;                           // fused.cu:164
#pragma unroll
        for (int j = 0; j < 16; j++) q[j] = quant_round_cuda(v[j], inv);
    } else {
        // x / scale must be the correctly rounded IEEE quotient (the reference divides, quant_per_block.py:41;
        // the +-0.5 / truncate that follows makes a 1-ulp error visible in the int8): sage_quant_math.h
        const float sc = quant_scale(am, style);
        const float y = quant_recip(sc);
        if (style == QS_TRITON_THREAD) {
#pragma unroll
            for (int j = 0; j < 16; j++) q[j] = quant_round_triton_nz(v[j], sc, y);
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) q[j] = quant_round_triton(v[j], sc, y);
        }
    }
    v4u pk;
#pragma unroll
    for (int w = 0; w < 4; w++) pk[w] = pack_int8x4(q[4 * w], q[4 * w + 1], q[4 * w + 2], q[4 * w + 3]);
    return pk;
}

// ---- FP8 V image -----------------------------------------------------------------------------------------------------
// per-channel scale and its reciprocal from the channel's abs-max (fused.cu:395)
__device__ __forceinline__ float fp8_v_scale(float am, float scale_max) { return am / scale_max; }
__device__ __forceinline__ float fp8_v_recp(float am, float scale_max) { return am > 0.0f ? scale_max / am : 0.0f; }

// One 16-byte piece of the tile image (sage_prep_v.hip): row d, physical chunk pc, from a 64-token tile of raw fp16 / bf16 rows in LDS (row
// pitch LDT, tokens behind the last valid one zero).  smooth: subtract `mean` from the first `valid` tokens, the padding stays zero.
template <int DT, int LDT>
__device__ __forceinline__ v4u fp8_v_image_piece(const uint16_t *tile, int d, int pc, float mean, float recp, bool smooth, int valid)
{
    const int ch = swz_chunk<64>(d, pc);                   // involution: physical <-> logical
    float f[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int tok = pv_token_of_position(16 * ch + j);
        float x = ld16<DT>(tile[tok * LDT + d]);
        if (smooth) x = (tok < valid) ? x - mean : 0.0f;   // padding stays zero
        x *= recp;
        f[j] = fminf(fmaxf(x, -448.0f), 448.0f);             // satfinite
    }
    v4u pk;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        int word = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w], f[4 * w + 1], 0, false);
        word = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w + 2], f[4 * w + 3], word, true);
        pk[w] = (unsigned)word;
    }
    return pk;
}

}  // namespace sage
