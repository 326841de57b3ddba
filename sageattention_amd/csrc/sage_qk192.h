// sage_qk192.h -- the FP8-PV route for 192-wide Q / K rows against 128-wide V rows (include/sage_qk192_gfx950.h): what its two
// units share -- the image formats, the parameter blocks and the launchers.  Nothing of the D = 64 / 128 family or of the head_dim = 256 route
// includes it, and it includes nothing of theirs but the device helpers of sage_common.h / sage_quant_math.h.
#pragma once
#include "sage_common.h"

namespace sage {

constexpr int QK192_DQK = 192;                         // channels of a Q / K row
constexpr int QK192_DV = 128;                          // channels of a V / O row
constexpr int QK192_PANEL_BYTES = BLKK * 64;           // one 64-channel panel of a K tile: 64 rows of 64 bytes = 4 KiB
constexpr int QK192_K_TILE_BYTES = BLKK * QK192_DQK;   // one 64-key K tile: three panels = 12 KiB
constexpr int QK192_V_TILE_BYTES = QK192_DV * BLKK;    // one 64-key V image: 128 channels x 64 e4m3 = 8 KiB
constexpr int QK192_CHUNK = 256;                       // tokens per workgroup of the statistics launch
constexpr int QK192_WS_PER_CHUNK = QK192_DQK + QK192_DV;      // floats of one chunk's statistics: 192 K sums, 128 V maxima
// two K slots and two V slots (why two); the epilogue's four 8-KiB output slabs reuse the first 32 KiB
constexpr int QK192_LDS_BYTES = 2 * QK192_K_TILE_BYTES + 2 * QK192_V_TILE_BYTES;

// K image: a tile is THREE PANELS of 64 channels; panel P holds bytes 64 P .. 64 P + 63 of all 64 rows as 64-byte rows, the 16-byte chunk
// c (0 .. 3) of row r at chunk c ^ (r >> 2 & 3) -- the family's 64-byte-row order (swz_chunk<64>).  A plain 192-byte row stride would start
// rows 4 apart on one bank (4 * 192 = 768 = 3 * 256) and hd256's chunk ^ (row & 15) needs 16 chunks per row; 12 are not a power of two.
// The QK^T operand read is "lane = key row r, fixed chunk C = 2 kk + g of the row's twelve": byte offset
//     (C >> 2) * 4096 + r * 64 + ((C & 3) ^ (r >> 2 & 3)) * 16.
// Its 16-byte slot inside the 256-byte bank row is  4 (r & 3) + ((C & 3) ^ (r >> 2 & 3)):  for a fixed C a bijection of r & 15.  A ds_read_b128
// serves 16 lanes at a time -- {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of each half wave, the two halves (g = 0 / 1) apart -- and either
// set's rows are 16 different values mod 16 (0-3, 12-15, 4-11 / 4-11, 0-3, 12-15): 16 different slots, all 64 banks once, no conflict.  The
// sub-tile (rows + 32) and the panel (+ 4096) move every lane by a multiple of 256 bytes and change nothing.
__host__ __device__ inline int qk192_k_offset(int row, int chunk)
{
    return (chunk >> 2) * QK192_PANEL_BYTES + row * 64 + swz_chunk<64>(row, chunk & 3) * 16;
}

// V image: channel d (0 .. 127) is 64 bytes in the PV "position" order of sage_common.h (byte p = token pv_token_of_position(p)), the chunk
// p >> 4 at (p >> 4) ^ (d >> 2 & 3).  The PV operand read is "lane = channel d = 32 dt + n, chunks 2 g and 2 g + 1": the argument above with
// d for r -- each of the two reads of a lane set hits 16 different slots.
__host__ __device__ inline int qk192_position_of_token(int t)
{
    return 32 * ((t >> 2) & 1) + 8 * (t >> 4) + 4 * ((t >> 3) & 1) + (t & 3);
}
__host__ __device__ inline int qk192_v_offset(int channel, int pos)
{
    return channel * 64 + swz_chunk<64>(channel, pos >> 4) * 16 + (pos & 15);
}

struct Qk192AttnParams {
    const void *q;                  // fp16 / bf16, rows of 192
    const unsigned char *k_img, *v_img;
    const float *k_scale, *v_scale;
    void *o;                        // rows of 128
    float *lse;                     // nullable
    long q_sb, q_sh, q_sl, o_sb, o_sh, o_sl;
    int B, Hq, Hkv, Lq, Lk, nqblk, ntile, group;
    float sm_scale_log2;
};

struct Qk192PrepParams {
    const void *k, *v;              // rows of 192 / of 128
    unsigned char *k_img, *v_img;
    float *k_scale, *v_scale, *ws;
    void *k_mean;                   // input dtype
    long k_sb, k_sh, k_sl, v_sb, v_sh, v_sl;
    int B, Hkv, Lk, ntile, nchunk, smooth_k;
};

hipError_t launch_qk192_attn(const Qk192AttnParams &p, bool causal, int dtype, hipStream_t stream);
hipError_t launch_qk192_prepass(const Qk192PrepParams &p, int dtype, hipStream_t stream);

}  // namespace sage
