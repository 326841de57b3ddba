// sage_chunk_max.h -- what the translation units of the exact split's pass 1 share (sage_split_exact.hip, sage_split_paged.hip): the row map of
// an MFMA tile and the fused-Q quantiser as a function.  Device code, included inside namespace-level scope of those units.
#pragma once
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_quant_math.h"
#include <climits>

namespace sage {

// c/d register r of a 32x32 MFMA tile -> row index inside the tile (lane half g), as sage_attn_kernel.h's crow
__device__ __forceinline__ int cm_crow(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }

// chunk_max_kernel's Q prologue as a function (that kernel keeps its own copy: its instruction stream stays what it was; with
// sage_attn_kernel.h's fused-Q prologue that makes THREE copies that must stay bit-equal -- change one, change all) -- the fused-Q
// prologue of sage_attn_kernel (QF 1 / 2) for the lane's row `qrow` (ok: the row exists, else zeros): per-thread groups = rows
// r, r+8, r+16, r+24 of the wave, both lane halves; the lane's INT8 fragments (channels 32 ks + 16 g .. + 15) and its group's scale
template <int D, int QDT>
__device__ __forceinline__ void cm_quant_q(const uint16_t *qrow, bool ok, int g, v4i (&qf)[D / 32], float &qsc)
{
    constexpr int KSTEPS = D / 32;
    float x[KSTEPS][16];
    float amax = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++) {
        v4u raw[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
        if (ok) {
            raw[0] = *reinterpret_cast<const v4u *>(qrow + 32 * ks + 16 * g);
            raw[1] = *reinterpret_cast<const v4u *>(qrow + 32 * ks + 16 * g + 8);
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const unsigned w = raw[j >> 3][(j & 7) >> 1];
            const float f = ld16<QDT>((uint16_t)((j & 1) ? (w >> 16) : (w & 0xffffu)));
            x[ks][j] = f;
            amax = fmaxf(amax, fabsf(f));
        }
    }
    amax = fmaxf(amax, __shfl_xor(amax, 8));
    amax = fmaxf(amax, __shfl_xor(amax, 16));
    amax = fmaxf(amax, __shfl_xor(amax, 32));
    const float sc = quant_scale(amax, QS_TRITON_THREAD);
    const float y = quant_recip(sc);
    qsc = sc;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++) {
        int q8[16];
#pragma unroll
        for (int j = 0; j < 16; j++) q8[j] = quant_round_triton_nz(x[ks][j], sc, y);
#pragma unroll
        for (int w = 0; w < 4; w++) qf[ks][w] = (int)pack_int8x4(q8[4 * w], q8[4 * w + 1], q8[4 * w + 2], q8[4 * w + 3]);
    }
}

}  // namespace sage
