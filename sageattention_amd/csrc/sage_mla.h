// sage_mla.h -- the FP8-PV route for the absorbed multi-head-latent-attention decode shape, 576-wide Q / K rows against the first 512 channels
// of the same latent rows as V (include/sage_mla_gfx950.h): what its two units share -- the image formats, the parameter blocks
// and the launchers.  It includes nothing of the other routes but the device helpers of sage_common.h / sage_quant_math.h.
#pragma once
#include "sage_common.h"
#include "sage_quant_math.h"

#include <atomic>

namespace sage {

constexpr int MLA_DQK = 576;                           // channels of a latent row: 512 compressed + 64 rope
constexpr int MLA_DV = 512;                            // channels of V and of an output row: the compressed ones
constexpr int MLA_PANEL_BYTES = BLKK * 64;             // one 64-channel panel of a K tile: 64 rows of 64 bytes = 4 KiB
constexpr int MLA_K_TILE_BYTES = BLKK * MLA_DQK;       // one 64-key K tile: nine panels = 36 KiB
constexpr int MLA_V_TILE_BYTES = MLA_DV * BLKK;        // one 64-key V tile: 512 channels x 64 e4m3 = 32 KiB
constexpr int MLA_CHUNK = 256;                         // tokens per workgroup of the statistics launch
constexpr int MLA_WS_PER_CHUNK = MLA_DQK + MLA_DV;     // floats of one chunk's statistics: 576 K sums, 512 V maxima
// two K slots and two V slots: 136 KiB, one workgroup per CU; the epilogue's four 32-KiB output slabs reuse the first 128 KiB
constexpr int MLA_LDS_BYTES = 2 * MLA_K_TILE_BYTES + 2 * MLA_V_TILE_BYTES;

// the statistics workspace of sample b: its chunks' 1088 floats each, then the 512 folded V maxima (the quantiser divides 448 by the amax
// itself, which v_scale = amax / 448 does not give back bit for bit)
__host__ __device__ inline long mla_ws_per_sample(int nchunk) { return (long)nchunk * MLA_WS_PER_CHUNK + MLA_DV; }

// K image: a tile is NINE PANELS of 64 channels in exactly the panel format of sage_qk192.h -- 64-byte rows, the 16-byte chunk c (0 .. 3) of
// row r at chunk c ^ (r >> 2 & 3).  The QK^T operand read is "lane = key row r, fixed chunk C of the row's 36" at
//     (C >> 2) * 4096 + r * 64 + ((C & 3) ^ (r >> 2 & 3)) * 16,
// and the bank argument written there carries over unchanged: the panel moves every lane by a multiple of 256 bytes.
__host__ __device__ inline int mla_k_offset(int row, int chunk)
{
    return (chunk >> 2) * MLA_PANEL_BYTES + row * 64 + swz_chunk<64>(row, chunk & 3) * 16;
}

// V image: channel d (0 .. 511) is 64 bytes in the PV "position" order of sage_common.h (byte p = token pv_token_of_position(p)), the chunk
// p >> 4 at (p >> 4) ^ (d >> 2 & 3).  The PV operand read is "lane = channel d = 32 dt + n, chunks 2 g and 2 g + 1".
__host__ __device__ inline int mla_position_of_token(int t)
{
    return 32 * ((t >> 2) & 1) + 8 * (t >> 4) + 4 * ((t >> 3) & 1) + (t & 3);
}
__host__ __device__ inline int mla_v_offset(int channel, int pos)
{
    return channel * 64 + swz_chunk<64>(channel, pos >> 4) * 16 + (pos & 15);
}

struct MlaAttnParams {
    const void *q;                  // fp16 / bf16 [B, Lq, Hq, 576] behind element strides
    const unsigned char *k_img, *v_img;
    const float *k_scale, *v_scale;
    const int32_t *kv_lens;         // nullable: every sample has Lk rows
    void *o;                        // [B, Lq, Hq, 512] contiguous
    float *lse;                     // nullable [B, Hq, Lq]
    long q_sb, q_sl, q_sh;
    int B, Lq, Hq, Lk, rows, nblk, ntile;       // rows = Lq * Hq, nblk = ceil(rows / 128)
    float sm_scale_log2;
};

struct MlaPrepParams {
    const void *kv;                 // [B, Lk, 576] behind element strides
    const int32_t *kv_lens;         // nullable
    unsigned char *k_img, *v_img;
    float *k_scale, *v_scale, *ws;
    void *k_mean;                   // input dtype
    long kv_sb, kv_sl;
    int B, Lk, ntile, nchunk, smooth_k;
};

// the valid rows of sample b (device side; the host never learns them)
__device__ __forceinline__ int mla_kv_len(const int32_t *kv_lens, int b, int Lk)
{
    const int n = kv_lens != nullptr ? kv_lens[b] : Lk;
    return n < 0 ? 0 : (n > Lk ? Lk : n);
}

hipError_t launch_mla_attn(const MlaAttnParams &p, int dtype, hipStream_t stream);
hipError_t launch_mla_prepass(const MlaPrepParams &p, int dtype, hipStream_t stream);

// host side of sage_mla_attn (sage_mla_attn.hip), shared with sage_mlasplit_attn (sage_mla_split.hip): the argument checks in front of the LDS
// check with the parameter block they allow, and the once-per-device opt-in to more than 64 KiB of dynamic LDS for `count` kernels
int mla_attn_prepare(const char *e, const void *q, const void *k_image, const void *v_image, const float *k_scale, const float *v_scale,
                     const int32_t *kv_lens, void *o, float *lse, int B, int Lq, int Hq, int Lk, int width_qk, int width_v, int64_t q_sb,
                     int64_t q_sl, int64_t q_sh, float sm_scale, int dtype, MlaAttnParams &p);
int mla_raise_lds(const char *e, std::atomic<unsigned long long> &done, int bytes, const void *const *kernels, const int *kernel_bytes, int count);

}  // namespace sage
