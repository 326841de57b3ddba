// sage_hd256.h -- the head_dim = 256 FP8-PV route (include/sage_hd256_gfx950.h): what its two units share -- the image
// formats, the parameter blocks and the launchers.  Nothing of the D = 64 / 128 kernel family includes it, and it includes nothing of the family's
// but the device helpers of sage_common.h / sage_quant_math.h.
#pragma once
#include "sage_common.h"

namespace sage {

constexpr int HD256 = 256;                        // the head size of the route
constexpr int HD256_TILE_BYTES = BLKK * HD256;    // one 64-key K tile (int8 rows) = one 64-key V image (256 channels x 64 e4m3) = 16 KiB
constexpr int HD256_CHUNK = 256;                  // tokens per workgroup of the statistics launch
constexpr int HD256_LDS_BYTES = 4 * HD256_TILE_BYTES;     // two K slots, two V slots; the epilogue's four 32-row output slabs

// K image: row r of a tile is 256 bytes, 16 chunks of 16 channels; chunk c stands at c ^ (r & 15).  The QK^T operand read is "lane = row,
// fixed chunk" over rows that are a whole 256-byte bank row apart: the XOR puts the 16 lanes of a ds_read_b128 group ({0-3, 12-15, 20-27} /
// {4-11, 16-19, 28-31}: their row indices mod 16 are all different) on 16 different 16-byte slots.
__host__ __device__ inline int hd256_k_chunk(int row, int chunk) { return chunk ^ (row & 15); }

// V image: channel d is 64 bytes in the PV "position" order of sage_common.h (byte p = token pv_token_of_position(p)), chunk-swizzled as the
// family's 64-byte rows are (swz_chunk<64>): the PV operand read "lane = channel, chunks 2 g and 2 g + 1" is conflict-free.
__host__ __device__ inline int hd256_position_of_token(int t)
{
    return 32 * ((t >> 2) & 1) + 8 * (t >> 4) + 4 * ((t >> 3) & 1) + (t & 3);
}

struct Hd256AttnParams {
    const void *q;                  // fp16 / bf16
    const unsigned char *k_img, *v_img;
    const float *k_scale, *v_scale;
    void *o;
    float *lse;                     // nullable
    long q_sb, q_sh, q_sl, o_sb, o_sh, o_sl;
    int B, Hq, Hkv, Lq, Lk, nqblk, ntile, group;
    float sm_scale_log2;
};

struct Hd256PrepParams {
    const void *k, *v;
    unsigned char *k_img, *v_img;
    float *k_scale, *v_scale, *ws;
    void *k_mean;                   // input dtype
    long k_sb, k_sh, k_sl, v_sb, v_sh, v_sl;
    int B, Hkv, Lk, ntile, nchunk, smooth_k;
};

hipError_t launch_hd256_attn(const Hd256AttnParams &p, bool causal, int dtype, hipStream_t stream);
hipError_t launch_hd256_prepass(const Hd256PrepParams &p, int dtype, hipStream_t stream);

}  // namespace sage
