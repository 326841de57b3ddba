// sage_qk192.h -- the FP8-PV route for 192-wide Q / K rows against 128-wide V rows (include/sage_qk192_gfx950.h): what its two
// units share -- the image formats, the parameter blocks and the launchers.  Nothing of the D = 64 / 128 family or of the head_dim = 256 route
// includes it, and it includes nothing of theirs but the device helpers of sage_common.h / sage_quant_math.h.
#pragma once
#include "sage_common.h"
#include "sage_quant_math.h"

#include <climits>
#include <type_traits>

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

// ---- the packed (variable-length) form of the route (include/sage_qk192v_gfx950.h) ----
// The plan, one int32 array at the head of the caller's workspace (sizes from nseq, total_q, total_k on the host; the true counts stay on the device):
//   hdr[8]             launch_varlen_plan's header: hdr[0] = work items
//   cnt[8]             cnt[0] = 64-key tiles, cnt[1] = 256-token statistics chunks, both clamped to the capacities below
//   cu_kt[nseq + 1]    tile prefix: sequence s owns tiles cu_kt[s] .. cu_kt[s + 1] - 1 of every kv head's images
//   cu_ch[nseq + 1]    statistics-chunk prefix
//   items[2 items_cap] (sequence, 128-row block), heaviest first            items_cap = ceil(total_q / 128) + nseq
//   kt_seq[tiles_cap]  tile -> sequence                                     tiles_cap = ceil(total_k / 64) + nseq
//   ch_seq[chunks_cap] chunk -> sequence                                    chunks_cap = ceil(total_k / 256) + nseq
// then, 16-byte aligned, the statistics [Hkv, chunks_cap, 320] floats.
struct Qk192vPlan {
    int nseq, items_cap, tiles_cap, chunks_cap;
    __host__ __device__ long hdr() const { return 0; }
    __host__ __device__ long cnt() const { return 8; }
    __host__ __device__ long cu_kt() const { return 16; }
    __host__ __device__ long cu_ch() const { return cu_kt() + nseq + 1; }
    __host__ __device__ long items() const { return cu_ch() + nseq + 1; }
    __host__ __device__ long kt_seq() const { return items() + 2L * items_cap; }
    __host__ __device__ long ch_seq() const { return kt_seq() + tiles_cap; }
    __host__ __device__ long ints() const { return (ch_seq() + chunks_cap + 3) & ~3L; }       // the floats behind stay 16-byte aligned
};
inline Qk192vPlan qk192v_plan(int nseq, int total_q, int total_k)
{
    return Qk192vPlan{nseq, (total_q + BLKQ - 1) / BLKQ + nseq, (total_k + BLKK - 1) / BLKK + nseq, (total_k + QK192_CHUNK - 1) / QK192_CHUNK + nseq};
}

constexpr int QK192_MASK_NONE = 0, QK192_MASK_TOP_LEFT = 1, QK192_MASK_BOTTOM_RIGHT = 2;

struct Qk192vPrepParams {
    const void *k, *v;              // [total_k, Hkv, 192] / [total_k, Hkv, 128] behind (token, head) strides
    const int32_t *cu_q, *cu_k;
    int32_t *plan;
    unsigned char *k_img, *v_img;   // [Hkv, tiles_cap, 12288] / [Hkv, tiles_cap, 8192]
    float *k_scale, *v_scale, *ws;  // [Hkv, 4 tiles_cap], [nseq, Hkv, 128], the statistics
    void *k_mean;                   // [nseq, Hkv, 192], input dtype
    long k_sl, k_sh, v_sl, v_sh;
    Qk192vPlan lay;
    int Hq, Hkv, total_q, total_k, mask, smooth_k;
};

struct Qk192vAttnParams {
    const void *q;                  // [total_q, Hq, 192] behind (token, head) strides
    const int32_t *cu_q, *cu_k, *plan;
    const unsigned char *k_img, *v_img;
    const float *k_scale, *v_scale;
    void *o;                        // [total_q, Hq, 128]
    float *lse;                     // nullable [Hq, total_q]
    long q_sl, q_sh, o_sl, o_sh;
    Qk192vPlan lay;
    int Hq, Hkv, group, total_q, total_k;
    float sm_scale_log2;
};

hipError_t launch_qk192v_prepass(const Qk192vPrepParams &p, int dtype, hipStream_t stream);
hipError_t launch_qk192v_attn(const Qk192vAttnParams &p, int mask, int dtype, hipStream_t stream);

// ---- one work item of the attention kernels: 128 query rows of one query head against the images of one (sequence, kv head) ----
// The dense kernel (sage_qk192_attn.hip, whose head comment describes the item) and the packed one (sage_qk192_varlen_attn.hip) differ in where
// an item's operands lie and in the causal diagonal; the tile loop with its counted waits is this one function.
struct Qk192Item {
    const uint16_t *q;              // row 0 of the (sequence, query head), rows q_sl elements apart
    unsigned char *o;               // row 0 of the output, rows o_sl elements apart
    float *lse;                     // row 0 of the head's LSE, nullable
    const unsigned char *k_img, *v_img;     // tile 0 of the (sequence, kv head)
    const float *k_scale, *v_scale;         // four per tile from tile 0; 128
    long q_sl, o_sl;
    int Lq, Lk, qblk;
    int shift;                      // QK192_MASK_BOTTOM_RIGHT: row i sees keys j <= i + shift
    float sm_scale_log2;
};

// hwreg(HW_REG_MODE, 23, 1): MODE.FP16_OVFL -- conversions saturate to the largest finite value
constexpr int kQk192ModeFp16Ovfl = 1 | (23 << 6) | (0 << 11);

// c/d register r of a 32x32 MFMA tile -> row index inside the tile (lane half g = lane >> 5)
__device__ __forceinline__ int qk192_crow(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }

// The caller promises an item with at least one visible key (kend >= 1): the prologue requests tile 0 unconditionally, and the counted waits
// below start from exactly that request.  Every thread of the workgroup calls it (raw barriers inside); smem: QK192_LDS_BYTES.
template <int MASK, int DT>
__device__ __forceinline__ void qk192_item(const Qk192Item &it, unsigned char *smem)
{
    constexpr bool CAUSAL = MASK != QK192_MASK_NONE;
    constexpr int DQK = QK192_DQK, DV = QK192_DV, KSTEPS = DQK / 32, NDT = DV / 32, KTB = QK192_K_TILE_BYTES, VTB = QK192_V_TILE_BYTES;
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int n = lane & 31, g = lane >> 5;
    __builtin_amdgcn_s_setreg(kQk192ModeFp16Ovfl, 1);

    const int shift = MASK == QK192_MASK_BOTTOM_RIGHT ? it.shift : 0;
    const int qblk = it.qblk;
    const int Lk = it.Lk, Lq = it.Lq;
    const int row0 = qblk * BLKQ + wave * 32;           // the wave's first query row
    const int my_row = row0 + n;
    const int kend = CAUSAL ? (Lk < qblk * BLKQ + BLKQ + shift ? Lk : qblk * BLKQ + BLKQ + shift) : Lk;
    const int n_tiles = (kend + BLKK - 1) / BLKK;       // >= 1, <= the tiles of the images
    const unsigned char *kimg = it.k_img;
    const unsigned char *vimg = it.v_img;
    typedef const __attribute__((address_space(4))) float *cfloat_p;       // K scales by scalar loads: a VGPR load would join the DMA's counter
    const cfloat_p ks_c = (cfloat_p)it.k_scale;

    // a tile = PIECES-per-wave x four waves of 1-KiB pieces (K: 3, V: 2); source and destination are lane-linear
    auto issue_tile = [&](const unsigned char *src_tile, unsigned char *slot, auto pieces_tag) {
        constexpr int PIECES = decltype(pieces_tag)::value;
        const unsigned char *src = src_tile + wave * (PIECES * 1024) + lane * 16;
#pragma unroll
        for (int i = 0; i < PIECES; i++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + i * 1024),
                                             (__attribute__((address_space(3))) void *)(slot + wave * (PIECES * 1024) + i * 1024), 16, 0, 0);
    };
    using KPieces = std::integral_constant<int, KTB / 4096>;     // 3
    using VPieces = std::integral_constant<int, VTB / 4096>;     // 2
    unsigned char *const kring = smem, *const vring = smem + 2 * KTB;
    issue_tile(kimg, kring, KPieces{});
    issue_tile(vimg, vring, VPieces{});

    // ---- Q: the lane's 16 channels of every k-step of its row, quantised per thread group (rows n, n + 8, n + 16, n + 24 of the wave, all
    //      channels: quant_per_thread.py:21-52) into the B operands ----
    v4i qf[KSTEPS];
    float qsc;
    {
        const uint16_t *qrow = it.q + (long)my_row * it.q_sl;
        const bool ok = my_row < Lq;
        // two passes over the row (the second hits the cache): the abs-max first, then k-step by k-step load, quantise and pack
        auto load16 = [&](int ks, float (&x)[16]) {
            v4u raw[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
            if (ok) {
                raw[0] = *reinterpret_cast<const v4u *>(qrow + 32 * ks + 16 * g);
                raw[1] = *reinterpret_cast<const v4u *>(qrow + 32 * ks + 16 * g + 8);
            }
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const unsigned w = raw[j >> 3][(j & 7) >> 1];
                x[j] = ld16<DT>((uint16_t)((j & 1) ? (w >> 16) : (w & 0xffffu)));
            }
        };
        float amax = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) {
            float x[16];
            load16(ks, x);
#pragma unroll
            for (int j = 0; j < 16; j++) amax = fmaxf(amax, fabsf(x[j]));
        }
        amax = fmaxf(amax, __shfl_xor(amax, 8));
        amax = fmaxf(amax, __shfl_xor(amax, 16));
        amax = fmaxf(amax, __shfl_xor(amax, 32));
        const float sc = quant_scale(amax, QS_TRITON_THREAD);
        const float y = quant_recip(sc);
        qsc = sc;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) {
            float x[16];
            load16(ks, x);
            int q8[16];
#pragma unroll
            for (int j = 0; j < 16; j++) q8[j] = quant_round_triton_nz(x[j], sc, y);
#pragma unroll
            for (int w = 0; w < 4; w++) qf[ks][w] = (int)pack_int8x4(q8[4 * w], q8[4 * w + 1], q8[4 * w + 2], q8[4 * w + 3]);
        }
    }

    v16f o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; dt++)
#pragma unroll
        for (int i = 0; i < 16; i++) o[dt][i] = 0.0f;
    float m_run = kNegBig, l_run = 0.0f;

    // the lane's two K scales of a tile: keys of registers with (i & 2) == 0 / != 0 lie in groups 2 g / 2 g + 1 of quant_per_thread.py:75-83
    // (all four by wave-uniform scalar loads, then a select: a per-lane choice of the ADDRESS would make them vector loads, and a vector load
    // waited for in the loop drags the tile DMA behind it in the in-order counter)
    auto k_scales = [&](int t, float &s0, float &s1) {
        const float a0 = ks_c[4 * t], a1 = ks_c[4 * t + 1], a2 = ks_c[4 * t + 2], a3 = ks_c[4 * t + 3];
        s0 = g ? a2 : a0;
        s1 = g ? a3 : a1;
    };
    float ksc0, ksc1;
    k_scales(0, ksc0, ksc1);

    // the lane's operand offsets inside a slot: K row n of sub-tile 0 (sub-tile 1 is 32 rows = 2048 bytes on, the same swizzle: 32 >> 2 & 3 == 0),
    // chunk (2 kk + g) & 3 = 2 (kk & 1) + g of panel kk >> 1; V channel n of output tile 0 (tile dt is 32 channels = 2048 bytes on)
    const int koff0 = n * 64 + swz_chunk<64>(n, g) * 16, koff1 = n * 64 + swz_chunk<64>(n, 2 + g) * 16;
    const int voff0 = n * 64 + swz_chunk<64>(n, 2 * g) * 16, voff1 = n * 64 + swz_chunk<64>(n, 2 * g + 1) * 16;

    for (int t = 0; t < n_tiles; t++) {
        const int slot = t & 1;
        const bool more = t + 1 < n_tiles;
        // vmcnt(2): the wave's DMA instructions still counted here are, oldest first, K of tile t (3) and V of tile t (2) -- requested in the
        // prologue (t = 0; the Q loads behind them were waited for by the prologue's own use of them) or behind the top barrier of tile
        // t - 1, whose PV wait left exactly these five.  The counter retires in order: at most 2 left means the three K pieces have landed
        // and V's two may still fly.  Then the barrier: everybody's K pieces.
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        float ksn0 = 0.0f, ksn1 = 0.0f;
        if (more) {
            issue_tile(kimg + (long)(t + 1) * KTB, kring + (slot ^ 1) * KTB, KPieces{});
            issue_tile(vimg + (long)(t + 1) * VTB, vring + (slot ^ 1) * VTB, VPieces{});
            k_scales(t + 1, ksn0, ksn1);
        }
        const int key0 = t * BLKK;
        const bool active = !CAUSAL || key0 <= row0 + 31 + shift;       // (wave-uniform) some row of the wave sees a key of the tile
        int pw[8];                                              // P of the tile: 32 e4m3 per lane, the B operand of PV
        float alpha = 1.0f;
        if (active) {
            const unsigned char *ks = kring + slot * KTB;
            // ---- S^T = K Q^T, two sub-tiles of 32 keys, six k-steps each: k-step kk reads chunk 2 kk + g of the row's twelve ----
            v16i s[2];
#pragma unroll
            for (int sb = 0; sb < 2; sb++) {
#pragma unroll
                for (int i = 0; i < 16; i++) s[sb][i] = 0;
#pragma unroll
                for (int kk = 0; kk < KSTEPS; kk++) {
                    const v4i a = *reinterpret_cast<const v4i *>(ks + (kk >> 1) * QK192_PANEL_BYTES + sb * 2048 + ((kk & 1) ? koff1 : koff0));
                    s[sb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, qf[kk], s[sb], 0, 0, 0);
                }
            }
            // the reference's order: sm_scale log2(e) * (q_scale * k_scale)  (qk_int_sv_f8_cuda_sm89.cuh:263-266)
            const float cs0 = it.sm_scale_log2 * (qsc * ksc0), cs1 = it.sm_scale_log2 * (qsc * ksc1);
            const bool full = (key0 + BLKK <= Lk) && (!CAUSAL || key0 + BLKK - 1 <= row0 + shift);
            // ---- row maximum: m_temp = fma(max score, scale, -offset) over the keys the row sees (attn_utils.cuh:372-384) ----
            float mx;
            if (full) {
                int mx0 = INT_MIN, mx1 = INT_MIN;
#pragma unroll
                for (int sb = 0; sb < 2; sb++)
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        if (i & 2) mx1 = max(mx1, s[sb][i]);
                        else mx0 = max(mx0, s[sb][i]);
                    }
                mx = fmaxf(__builtin_fmaf((float)mx0, cs0, -kFp8Offset), __builtin_fmaf((float)mx1, cs1, -kFp8Offset));
            } else {
                mx = -INFINITY;
#pragma unroll
                for (int sb = 0; sb < 2; sb++)
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        const int key = key0 + sb * 32 + qk192_crow(i, g);
                        const bool ok = key < Lk && (!CAUSAL || key <= my_row + shift);
                        mx = fmaxf(mx, ok ? __builtin_fmaf((float)s[sb][i], (i & 2) ? cs1 : cs0, -kFp8Offset) : -INFINITY);
                    }
            }
            // (a row that has seen no key yet -- bottom-right with more rows than keys -- keeps m_run = kNegBig: alpha = exp2(0) = 1, its
            // exp2 below overflows to +inf and the mask turns it into 0 BEFORE the row sum; `full` is never true for such a row's wave)
            const float m_new = fmaxf(m_run, pair_max(mx));
            alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
            // ---- P: chunk c (16 keys) = registers 8 (c & 1) .. + 7 of sub-tile c >> 1, the order of the PV operand (sage_common.h) ----
            float rs = 0.0f;
            auto build_p = [&](auto masked) {
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int sb = c >> 1, r0 = (c & 1) * 8;
                    float e[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int i = r0 + j;
                        float v = __builtin_amdgcn_exp2f(__builtin_fmaf((float)s[sb][i], (i & 2) ? cs1 : cs0, -m_new));
                        if constexpr (decltype(masked)::value) {
                            const int key = key0 + sb * 32 + qk192_crow(i, g);
                            v = (key < Lk && (!CAUSAL || key <= my_row + shift)) ? v : 0.0f;
                        }
                        e[j] = v;
                        rs += v;
                    }
                    int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[0], e[1], 0, false);
                    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[2], e[3], w0, true);
                    int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[4], e[5], 0, false);
                    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[6], e[7], w1, true);
                    pw[2 * c] = w0;
                    pw[2 * c + 1] = w1;
                }
            };
            if (full) build_p(std::false_type{});
            else build_p(std::true_type{});
            l_run = l_run * alpha + rs;          // lane-partial; the lane pair is summed in the epilogue
        }
        // vmcnt(5) / vmcnt(0): behind the top wait the wave's counted DMA instructions are, oldest first, V of tile t (2) and, if there is a
        // next tile, its K (3) and V (2) requested above.  At most 3 + 2 = 5 left means V of tile t has landed with the whole next tile
        // still in flight; on the last tile nothing younger exists and the wait is for zero.  Then the barrier: everybody's V pieces.
        if (more) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (active) {
            const unsigned char *vs = vring + slot * VTB;
            const v8i bv = {pw[0], pw[1], pw[2], pw[3], pw[4], pw[5], pw[6], pw[7]};
            const bool moved = __builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0;      // (wave-uniform)
            auto pv = [&](auto fold_tag) {
                constexpr bool FOLD = decltype(fold_tag)::value;
#pragma unroll
                for (int dt = 0; dt < NDT; dt++) {
                    const v4u va = *reinterpret_cast<const v4u *>(vs + dt * 2048 + voff0);
                    const v4u vb = *reinterpret_cast<const v4u *>(vs + dt * 2048 + voff1);
                    const v8i av = {(int)va[0], (int)va[1], (int)va[2], (int)va[3], (int)vb[0], (int)vb[1], (int)vb[2], (int)vb[3]};
                    if constexpr (FOLD) {
                        v16f acc;
#pragma unroll
                        for (int i = 0; i < 16; i++) acc[i] = 0.0f;
                        acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 0, 0, 0, 0, 0, 0);      // (zero scale operands: the plain form)
#pragma unroll
                        for (int i = 0; i < 16; i++) o[dt][i] = __builtin_fmaf(o[dt][i], alpha, acc[i]);
                    } else {
                        o[dt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, o[dt], 0, 0, 0, 0, 0, 0);
                    }
                }
            };
            if (moved) pv(std::true_type{});
            else pv(std::false_type{});
        }
        ksc0 = ksn0;
        ksc1 = ksn1;
    }
    __syncthreads();          // every wave is past its last operand read: the ring is free for the output slabs

    // ---- epilogue: normalise, times the V scale, cast, transpose through LDS, store rows ----
    __builtin_amdgcn_s_setreg(kQk192ModeFp16Ovfl, 0);
    const float l_tot = pair_sum(l_run);
    const float inv = l_tot > 0.0f ? __builtin_amdgcn_rcpf(l_tot) : 0.0f;
    if (it.lse != nullptr && g == 0 && my_row < Lq)
        it.lse[my_row] = __builtin_amdgcn_logf(l_tot) + m_run;      // v_log_f32 is log2
    unsigned char *obuf = smem + wave * (32 * DV * 2);       // 8 KiB per wave, 32 KiB of the ring's 40
    const float *vsc = it.v_scale;
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) {
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) {
            const int d0 = dt * 32 + 8 * r4 + 4 * g;           // four consecutive channels: registers 4 r4 .. 4 r4 + 3
            const v4f sc4 = *reinterpret_cast<const v4f *>(vsc + d0);
            unsigned short hx[4];
#pragma unroll
            for (int j = 0; j < 4; j++) hx[j] = st16<DT>(o[dt][4 * r4 + j] * inv * sc4[j]);
            v2u pk;
            pk[0] = (unsigned)hx[0] | ((unsigned)hx[1] << 16);
            pk[1] = (unsigned)hx[2] | ((unsigned)hx[3] << 16);
            const int q8 = d0 >> 2;                             // 8-byte chunk of the 256-byte row
            const int Q = (q8 >> 1) ^ (n & 15);                 // its 16-byte chunk of sixteen, XOR-ed by the row
            *reinterpret_cast<v2u *>(obuf + n * (DV * 2) + Q * 16 + (q8 & 1) * 8) = pk;
        }
    }
    // (the wave's own slab: its writes and reads execute in order, no workgroup barrier)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    unsigned char *obase = it.o;
#pragma unroll
    for (int pass = 0; pass < 8; pass++) {                      // 16 lanes of 16 bytes per row, four rows per pass
        const int r = 4 * pass + (lane >> 4), Q = lane & 15;
        const v4u val = *reinterpret_cast<const v4u *>(obuf + r * (DV * 2) + (Q ^ (r & 15)) * 16);
        const int grow = row0 + r;
        if (grow < Lq) *reinterpret_cast<v4u *>(obase + 2 * ((long)grow * it.o_sl) + Q * 16) = val;
    }
}

}  // namespace sage
