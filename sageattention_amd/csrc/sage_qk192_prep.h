// sage_qk192_prep.h -- the pre-pass of the 192-wide Q / K, 128-wide V route as the work of ONE workgroup: the statistics of a 256-token chunk and
// the images of a 64-key tile of one (sequence, kv head).  The dense launch (sage_qk192_prepass.hip) and the packed one
// (sage_qk192_varlen_prepass.hip) call these with a sequence's first token and its length; chunks and tiles count from that token, so a packed
// sequence gets bit for bit the statistics and images of a dense call on its slice (DESIGN 3.27 "Pre-pass", 3.28).
// Thread mappings: K rows are 24 columns of 8 channels (16-byte loads) and V rows 16, so the statistics run 8 row groups x 24 columns on threads
// 0 .. 191 for K and 16 row groups x 16 columns on all 256 for V; the quantiser gives a K row to four threads of 48 channels (three 16-byte
// chunks of the image each) and deals the 64 x 16 V columns of a tile four to a thread.
#pragma once
#include "sage_qk192.h"

namespace sage {

// eight consecutive channels of one row: a 16-byte load, zeros for a row past the last token
template <int DT>
__device__ __forceinline__ void qk192_load8(const uint16_t *row, bool ok, float (&x)[8])
{
    v4u raw = {0u, 0u, 0u, 0u};
    if (ok) raw = *reinterpret_cast<const v4u *>(row);
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = ld16<DT>((uint16_t)((j & 1) ? (raw[j >> 1] >> 16) : (raw[j >> 1] & 0xffffu)));
}

// kb / vb: token 0 of the (sequence, kv head), tokens k_sl / v_sl elements apart, Lk of them; w: the chunk's 320 floats
template <int DT>
__device__ __forceinline__ void qk192_stats_chunk(const uint16_t *kb, const uint16_t *vb, long k_sl, long v_sl, int chunk, int Lk, float *w)
{
    __shared__ float red_k[8][QK192_DQK], red_v[16][QK192_DV];
    const int tid = threadIdx.x;
    // ---- K: threads 0 .. 191 = (row group of 8, 8-channel column of 24): rows rg, rg + 8, .. of the chunk ----
    if (tid < 192) {
        const int cl = tid % 24, rg = tid / 24;
        float ksum[8];
#pragma unroll
        for (int j = 0; j < 8; j++) ksum[j] = 0.0f;
        for (int i = 0; i < QK192_CHUNK / 8; i++) {
            const int tok = chunk * QK192_CHUNK + 8 * i + rg;
            float kx[8];
            qk192_load8<DT>(kb + 8 * cl + (long)tok * k_sl, tok < Lk, kx);
#pragma unroll
            for (int j = 0; j < 8; j++) ksum[j] += kx[j];
        }
#pragma unroll
        for (int j = 0; j < 8; j++) red_k[rg][8 * cl + j] = ksum[j];
    }
    // ---- V: all threads = (row group of 16, 8-channel column of 16): rows rg, rg + 16, .. ----
    {
        const int cl = tid & 15, rg = tid >> 4;
        float vam[8];
#pragma unroll
        for (int j = 0; j < 8; j++) vam[j] = 0.0f;
        for (int i = 0; i < QK192_CHUNK / 16; i++) {
            const int tok = chunk * QK192_CHUNK + 16 * i + rg;
            float vx[8];
            qk192_load8<DT>(vb + 8 * cl + (long)tok * v_sl, tok < Lk, vx);
#pragma unroll
            for (int j = 0; j < 8; j++) vam[j] = fmaxf(vam[j], fabsf(vx[j]));
        }
#pragma unroll
        for (int j = 0; j < 8; j++) red_v[rg][8 * cl + j] = vam[j];
    }
    __syncthreads();
    // the row groups in ascending order: one fixed order of additions per channel
    if (tid < QK192_DQK) {
        float s = 0.0f;
#pragma unroll
        for (int r = 0; r < 8; r++) s += red_k[r][tid];
        w[tid] = s;
    } else {                                             // threads 192 .. 255: two V channels each
        for (int d = tid - QK192_DQK; d < QK192_DV; d += 64) {
            float a = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; r++) a = fmaxf(a, red_v[r][d]);
            w[QK192_DQK + d] = a;
        }
    }
}

// where a tile's workgroup writes: the (sequence, kv head)'s mean and V scale (tile 0 writes them), the tile's four K scales and its two images
struct Qk192TileOut {
    uint16_t *k_mean;
    float *v_scale, *k_scale;
    unsigned char *k_img, *v_img;
};

// w: the nchunk chunks' statistics of the (sequence, kv head), 320 floats apart, folded in ascending order
template <int DT>
__device__ __forceinline__ void qk192_quant_tile(const uint16_t *kb, const uint16_t *vb, long k_sl, long v_sl, int tile, int Lk,
                                                 const float *w, int nchunk, bool smooth_k, const Qk192TileOut &out)
{
    __shared__ float s_mean[QK192_DQK], s_vrecp[QK192_DV], s_ramax[BLKK];
    __shared__ __attribute__((aligned(16))) unsigned char s_img[QK192_V_TILE_BYTES];
    const int tid = threadIdx.x;

    // ---- the statistics of the (sequence, kv head): thread = channel, chunks in ascending order ----
    if (tid < QK192_DQK) {
        float s = 0.0f;
        for (int c = 0; c < nchunk; c++) s += w[(long)c * QK192_WS_PER_CHUNK + tid];
        // the reference's mean is the FP32 sum over Lk, rounded to the input dtype (core.py:773); without smooth_k nothing is subtracted
        const uint16_t m16 = smooth_k ? st16<DT>(s / (float)Lk) : (uint16_t)0;
        s_mean[tid] = ld16<DT>(m16);
        if (tile == 0) out.k_mean[tid] = m16;
    } else {
        for (int d = tid - QK192_DQK; d < QK192_DV; d += 64) {
            float a = 0.0f;
            for (int c = 0; c < nchunk; c++) a = fmaxf(a, w[(long)c * QK192_WS_PER_CHUNK + QK192_DQK + d]);
            s_vrecp[d] = a > 0.0f ? 448.0f / a : 0.0f;          // (a channel of zeros -- head_dim padding -- gives zero bytes, not 0 * inf)
            if (tile == 0) out.v_scale[d] = a / 448.0f;
        }
    }
    __syncthreads();

    // ---- K: thread = (row r of 64, quarter qd of the row: channels 48 qd .. 48 qd + 47, the image's chunks 3 qd .. 3 qd + 2) ----
    {
        const int r = tid >> 2, qd = tid & 3;
        const int key = tile * BLKK + r;
        const bool ok = key < Lk;
        const uint16_t *row = kb + (long)key * k_sl + 48 * qd;
        float x[48];
        float amax = 0.0f;
#pragma unroll
        for (int v = 0; v < 6; v++) {
            float f[8];
            qk192_load8<DT>(row + 8 * v, ok, f);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                // k - mean in the input dtype (core.py:775), as the reference's quantiser receives it
                const float d = smooth_k ? ld16<DT>(st16<DT>(f[j] - s_mean[48 * qd + 8 * v + j])) : f[j];
                x[8 * v + j] = ok ? d : 0.0f;
                amax = fmaxf(amax, fabsf(x[8 * v + j]));
            }
        }
        amax = fmaxf(amax, __shfl_xor(amax, 1));
        amax = fmaxf(amax, __shfl_xor(amax, 2));
        if (qd == 0) s_ramax[r] = amax;
        __syncthreads();
        // per-thread scale groups (quant_per_thread.py:75-83): group j of the tile = rows with (row % 8) / 2 == j
        auto group_scale = [&](int j) {
            float gm = 0.0f;
#pragma unroll
            for (int a = 0; a < 8; a++) gm = fmaxf(gm, fmaxf(s_ramax[8 * a + 2 * j], s_ramax[8 * a + 2 * j + 1]));
            return quant_scale(gm, QS_TRITON_THREAD);
        };
        if (tid < 4) out.k_scale[tid] = group_scale(tid);
        const float sc = group_scale((r & 7) >> 1);
        const float y = quant_recip(sc);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v4u pk;
#pragma unroll
            for (int w4 = 0; w4 < 4; w4++) {
                int q8[4];
#pragma unroll
                for (int j = 0; j < 4; j++) q8[j] = quant_round_triton_nz(x[16 * c + 4 * w4 + j], sc, y);
                pk[w4] = pack_int8x4(q8[0], q8[1], q8[2], q8[3]);
            }
            *reinterpret_cast<v4u *>(out.k_img + qk192_k_offset(r, 3 * qd + c)) = pk;
        }
    }

    // ---- V: 64 rows of sixteen 16-byte loads, e4m3 bytes scattered into the image in LDS, the image copied out linearly ----
    {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int e = tid + 256 * i, t = e >> 4, cv = e & 15;
            const int tok = tile * BLKK + t;
            float f[8];
            qk192_load8<DT>(vb + (long)tok * v_sl + 8 * cv, tok < Lk, f);
            const int pos = qk192_position_of_token(t);
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const int d = 8 * cv + j;
                const int w2 = __builtin_amdgcn_cvt_pk_fp8_f32(f[j] * s_vrecp[d], f[j + 1] * s_vrecp[d + 1], 0, false);
                s_img[qk192_v_offset(d, pos)] = (unsigned char)(w2 & 0xff);
                s_img[qk192_v_offset(d + 1, pos)] = (unsigned char)((w2 >> 8) & 0xff);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int e = tid + 256 * i;
            *reinterpret_cast<v4u *>(out.v_img + e * 16) = *reinterpret_cast<const v4u *>(s_img + e * 16);
        }
    }
}

}  // namespace sage
