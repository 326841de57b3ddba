// sage_mla_loop.h -- the device code that the attention kernel of the absorbed MLA decode shape (sage_mla_attn.hip) shares with
// its exact split of the key range (sage_mla_split.hip): the Q quantiser of the prologue, the LDS-DMA request of a tile, the
// QK^T of a tile with its row maximum, and the whole body of the attention kernel as mla_decode_body<DT, SPLIT>.
//
// SPLIT = false is the kernel of 3.29, statement for statement: every `if constexpr (SPLIT)` below folds away, and the compiler's resource line
// of mla_decode_kernel (256 VGPRs + 256 AGPRs, no scratch) is the one it had before this header existed.  SPLIT = true is pass 2 of 3.30: the
// work item carries a chunk c of T tiles, the PROLOGUE moves the image and scale pointers by T c tiles and the key limits into the chunk's
// coordinates (minus 64 T c), m_run starts at the maximum of the earlier chunks' maxima (pass 1 wrote them), and the EPILOGUE stores the FP32
// partial O (1 / l) v_scale with log2(l) + m instead of the cast result.  The loop between them is the same text for both.
#pragma once
#include "sage_mla.h"

#include <climits>
#include <type_traits>

namespace sage {

// hwreg(HW_REG_MODE, 23, 1): MODE.FP16_OVFL -- conversions saturate to the largest finite value
constexpr int kMlaModeFp16Ovfl = 1 | (23 << 6) | (0 << 11);

// c/d register r of a 32x32 MFMA tile -> row index inside the tile (lane half g = lane >> 5)
__device__ __forceinline__ int mla_crow(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }

// the split call: the attention call's parameters, the three workspace segments and the chunking.  Chunk c of sample b holds the tiles
// [T c, T c + T) of the sample; chunk_max and lse_part are [B, S, rows], o_part [B, S, rows, 512], all FP32.
struct MlaSplitParams {
    MlaAttnParams a;
    float *chunk_max, *lse_part, *o_part;
    int S, T;
};
__device__ __forceinline__ const MlaAttnParams &mla_attn_params(const MlaAttnParams &p) { return p; }
__device__ __forceinline__ const MlaAttnParams &mla_attn_params(const MlaSplitParams &p) { return p.a; }

typedef const __attribute__((address_space(4))) float *mla_cfloat_p;       // K scales by scalar loads: a VGPR load would join the DMA's counter

// a tile = PIECES-per-wave x four waves of 1-KiB pieces (K: 9, V: 8); source and destination are lane-linear
template <int PIECES>
__device__ __forceinline__ void mla_issue_tile(const unsigned char *src_tile, unsigned char *slot, int wave, int lane)
{
    const unsigned char *src = src_tile + wave * (PIECES * 1024) + lane * 16;
#pragma unroll
    for (int i = 0; i < PIECES; i++)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + i * 1024),
                                         (__attribute__((address_space(3))) void *)(slot + wave * (PIECES * 1024) + i * 1024), 16, 0, 0);
}
constexpr int MLA_K_PIECES = MLA_K_TILE_BYTES / 4096;     // 9
constexpr int MLA_V_PIECES = MLA_V_TILE_BYTES / 4096;     // 8

// ---- Q: the lane's 16 channels of every k-step of its row, INT8 with one scale per row, into the B operands ----
template <int DT>
__device__ __forceinline__ void mla_quantise_q(const uint16_t *qrow, bool row_ok, int g, v4i (&qf)[MLA_DQK / 32], float &qsc)
{
    constexpr int KSTEPS = MLA_DQK / 32;
    // two passes over the row (the second hits the cache): the abs-max first, then k-step by k-step load, quantise and pack
    auto load16 = [&](int ks, float (&x)[16]) {
        v4u raw[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
        if (row_ok) {
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
    amax = pair_max(amax);                          // the row's two lanes: the row is its own group
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

// the lane's two K scales of a tile: keys of registers with (i & 2) == 0 / != 0 lie in groups 2 g / 2 g + 1 of quant_per_thread.py:75-83
__device__ __forceinline__ void mla_k_scales(mla_cfloat_p ks_c, int t, int g, float &s0, float &s1)
{
    const float a0 = ks_c[4 * t], a1 = ks_c[4 * t + 1], a2 = ks_c[4 * t + 2], a3 = ks_c[4 * t + 3];
    s0 = g ? a2 : a0;
    s1 = g ? a3 : a1;
}

// ---- S^T = K Q^T, two sub-tiles of 32 keys, eighteen k-steps each: k-step kk reads chunk 2 kk + g of the row's 36 ----
__device__ __forceinline__ void mla_tile_scores(const unsigned char *ks, int koff0, int koff1, const v4i (&qf)[MLA_DQK / 32], v16i (&s)[2])
{
#pragma unroll
    for (int sb = 0; sb < 2; sb++) {
#pragma unroll
        for (int i = 0; i < 16; i++) s[sb][i] = 0;
#pragma unroll
        for (int kk = 0; kk < MLA_DQK / 32; kk++) {
            const v4i a = *reinterpret_cast<const v4i *>(ks + (kk >> 1) * MLA_PANEL_BYTES + sb * 2048 + ((kk & 1) ? koff1 : koff0));
            s[sb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, qf[kk], s[sb], 0, 0, 0);
        }
    }
}

// ---- row maximum: m_temp = fma(max score, scale, -offset) over the keys the row sees (attn_utils.cuh:372-384), lane-partial ----
// `full` (wave-uniform): every row of the wave sees the whole tile -- the integer maximum per K-scale group, one fma per group.  Otherwise the
// fma per score behind the mask.  Pass 1 of the split forms a chunk's maximum with THIS function, which is why its bits are the loop's.
__device__ __forceinline__ float mla_tile_max(const v16i (&s)[2], bool full, int key0, int lim, int g, float cs0, float cs1)
{
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
                const int key = key0 + sb * 32 + mla_crow(i, g);
                mx = fmaxf(mx, key <= lim ? __builtin_fmaf((float)s[sb][i], (i & 2) ? cs1 : cs0, -kFp8Offset) : -INFINITY);
            }
    }
    return mx;
}

// the work item of a split launch: block index -> (item of the unsplit grid, chunk), chunks of one item side by side
__device__ __forceinline__ void mla_split_item(const MlaSplitParams &pp, int &item, int &c)
{
    c = (int)blockIdx.x % pp.S;
    item = (int)blockIdx.x / pp.S;
}

template <int DT, bool SPLIT, class Params>
__device__ __forceinline__ void mla_decode_body(const Params &pp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const MlaAttnParams &p = mla_attn_params(pp);
    constexpr int DQK = MLA_DQK, DV = MLA_DV, KSTEPS = DQK / 32, NDT = DV / 32, KTB = MLA_K_TILE_BYTES, VTB = MLA_V_TILE_BYTES;
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int n = lane & 31, g = lane >> 5;

    // ---- work item: (sample, 128-row block of its [Lq * Hq] rows), split: and the chunk c of T tiles from tile0 on ----
    int item = (int)blockIdx.x, c = 0, tile0 = 0;
    if constexpr (SPLIT) {
        mla_split_item(pp, item, c);
        tile0 = c * pp.T;
    }
    const int b = item / p.nblk, blk = item % p.nblk;
    const int R = p.rows, Hq = p.Hq, Lq = p.Lq;
    const int kvlen = mla_kv_len(p.kv_lens, b, p.Lk);
    // the row at position i sees keys j <= i + shift; split: j counts from the chunk's first key, the mask itself stays the global one
    const int shift = kvlen - Lq - tile0 * BLKK;
    const int blk_last = (blk * BLKQ + BLKQ < R ? blk * BLKQ + BLKQ : R) - 1;          // the item's last valid row
    int kend = blk_last / Hq + shift + 1;                               // its limit + 1; at most kvlen
    // split: the chunk ends at its T-th tile.  Clamping kend alone is the whole clamp: no tile behind it is walked, so a key index stays
    // below 64 T and `key <= lim` needs no upper bound on lim; a limit below 0 is a row in front of the chunk's first key, as in front of key 0
    if constexpr (SPLIT) kend = kend < pp.T * BLKK ? kend : pp.T * BLKK;
    unsigned char *const obase = reinterpret_cast<unsigned char *>(p.o) + 2 * ((long)b * R * DV);
    float *const lse_b = p.lse != nullptr ? p.lse + (long)b * Hq * Lq : nullptr;
    long part_row0 = 0;                                                 // split: row 0 of (b, c) in the [B, S, rows] segments
    if constexpr (SPLIT) part_row0 = ((long)b * pp.S + c) * R;

    if (kend <= 0) {            // (workgroup-uniform) no row of the item sees a key: o = +0, lse = -inf, and nothing was requested
        const int nrow = blk_last - blk * BLKQ + 1;
        if constexpr (SPLIT) {  // split: no key of the CHUNK; lse_part = -inf is what makes the merge skip the chunk's o_part, left unwritten
            // (the thread index from wave and lane, which live on anyway: threadIdx.x itself cost the loop a spilled register)
            if (wave * 64 + lane < nrow) pp.lse_part[part_row0 + blk * BLKQ + wave * 64 + lane] = -INFINITY;
            return;
        }
        const v4u z = {0u, 0u, 0u, 0u};
        for (int e = (int)threadIdx.x; e < nrow * (DV / 8); e += 256)
            *reinterpret_cast<v4u *>(obase + 2 * ((long)(blk * BLKQ + e / (DV / 8)) * DV) + (e % (DV / 8)) * 16) = z;
        if (lse_b != nullptr && (int)threadIdx.x < nrow) {
            const int r = blk * BLKQ + (int)threadIdx.x;
            lse_b[(long)(r % Hq) * Lq + r / Hq] = -INFINITY;
        }
        return;
    }
    __builtin_amdgcn_s_setreg(kMlaModeFp16Ovfl, 1);

    const int n_tiles = (kend + BLKK - 1) / BLKK;       // >= 1, <= the tiles the pre-pass wrote for the sample (split: from tile0 on)
    const unsigned char *kimg = p.k_img + ((long)b * p.ntile + tile0) * KTB;
    const unsigned char *vimg = p.v_img + ((long)b * p.ntile + tile0) * VTB;
    const mla_cfloat_p ks_c = (mla_cfloat_p)(p.k_scale + ((long)b * p.ntile + tile0) * 4);

    unsigned char *const kring = smem, *const vring = smem + 2 * KTB;
    mla_issue_tile<MLA_K_PIECES>(kimg, kring, wave, lane);
    mla_issue_tile<MLA_V_PIECES>(vimg, vring, wave, lane);

    // ---- the wave's rows ----
    const int row0 = blk * BLKQ + wave * 32;            // the wave's first row
    const int my_row = row0 + n;
    const bool row_ok = my_row < R;
    const int crow = row_ok ? my_row : R - 1;           // (a row past the last borrows the last one's limit; it is never stored)
    const int my_pos = crow / Hq, my_head = crow % Hq;
    const int lim = my_pos + shift;                     // the lane's row sees keys j <= lim (< kvlen)
    const bool wave_ok = row0 < R;                      // (wave-uniform)
    const int lim_lo = (wave_ok ? row0 / Hq : 0) + shift;                               // the smallest limit of the wave's rows
    const int lim_hi = (row0 + 31 < R ? (row0 + 31) / Hq : (R - 1) / Hq) + shift;       // and the largest

    v4i qf[KSTEPS];
    float qsc;
    mla_quantise_q<DT>(reinterpret_cast<const uint16_t *>(p.q) + (long)b * p.q_sb + (long)my_pos * p.q_sl + (long)my_head * p.q_sh, row_ok, g, qf,
                       qsc);

    v16f o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; dt++)
#pragma unroll
        for (int i = 0; i < 16; i++) o[dt][i] = 0.0f;
    float m_run = kNegBig, l_run = 0.0f;
    if constexpr (SPLIT) {
        // the seed: what m_run is in the unsplit call when it reaches this chunk's first tile -- fmaxf over the earlier chunks' maxima, each
        // formed by pass 1 with mla_tile_max.  Chunk 0 starts where the unsplit kernel starts.  (Vector loads: consumed here, in front of the
        // loop, so the loop's counted waits see the DMA pieces alone.)
        const float *cm = pp.chunk_max + (long)b * pp.S * R + my_row;
        if (row_ok)
            for (int cc = 0; cc < c; cc++) m_run = fmaxf(m_run, cm[(long)cc * R]);
        asm volatile("" : "+v"(m_run));
    }

    float ksc0, ksc1;
    mla_k_scales(ks_c, 0, g, ksc0, ksc1);

    // the lane's operand offsets inside a slot: K row n of sub-tile 0 (sub-tile 1 is 32 rows = 2048 bytes on, the same swizzle), chunk
    // (2 kk + g) & 3 = 2 (kk & 1) + g of panel kk >> 1; V channel n of output tile 0 (tile dt is 32 channels = 2048 bytes on)
    const int koff0 = n * 64 + swz_chunk<64>(n, g) * 16, koff1 = n * 64 + swz_chunk<64>(n, 2 + g) * 16;
    const int voff0 = n * 64 + swz_chunk<64>(n, 2 * g) * 16, voff1 = n * 64 + swz_chunk<64>(n, 2 * g + 1) * 16;

    for (int t = 0; t < n_tiles; t++) {
        const int slot = t & 1;
        const bool more = t + 1 < n_tiles;
        // vmcnt(8): K of tile t (9, the older) has landed, V of tile t (8) may still fly -- sage_mla_attn.hip's head comment has the count
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        float ksn0 = 0.0f, ksn1 = 0.0f;
        if (more) {
            mla_issue_tile<MLA_K_PIECES>(kimg + (long)(t + 1) * KTB, kring + (slot ^ 1) * KTB, wave, lane);
            mla_issue_tile<MLA_V_PIECES>(vimg + (long)(t + 1) * VTB, vring + (slot ^ 1) * VTB, wave, lane);
            mla_k_scales(ks_c, t + 1, g, ksn0, ksn1);
        }
        const int key0 = t * BLKK;
        const bool active = wave_ok && key0 <= lim_hi;          // (wave-uniform) some row of the wave sees a key of the tile
        int pw[8];                                              // P of the tile: 32 e4m3 per lane, the B operand of PV
        float alpha = 1.0f;
        if (active) {
            v16i s[2];
            mla_tile_scores(kring + slot * KTB, koff0, koff1, qf, s);
            // the reference's order: sm_scale log2(e) * (q_scale * k_scale)  (qk_int_sv_f8_cuda_sm89.cuh:263-266)
            const float cs0 = p.sm_scale_log2 * (qsc * ksc0), cs1 = p.sm_scale_log2 * (qsc * ksc1);
            const bool full = key0 + BLKK - 1 <= lim_lo;        // (wave-uniform) every row of the wave sees the whole tile
            const float mx = mla_tile_max(s, full, key0, lim, g, cs0, cs1);
            // (a row that has seen no key yet keeps m_run = kNegBig: alpha = exp2(0) = 1, its exp2 below overflows to +inf and the mask turns
            // it into 0 BEFORE the row sum; `full` is never true for such a row's wave)
            const float m_new = fmaxf(m_run, pair_max(mx));
            alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
            // ---- P: chunk c (16 keys) = registers 8 (c & 1) .. + 7 of sub-tile c >> 1, the order of the PV operand (sage_common.h) ----
            float rs = 0.0f;
            auto build_p = [&](auto masked) {
#pragma unroll
                for (int ch = 0; ch < 4; ch++) {
                    const int sb = ch >> 1, r0 = (ch & 1) * 8;
                    float e[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int i = r0 + j;
                        float v = __builtin_amdgcn_exp2f(__builtin_fmaf((float)s[sb][i], (i & 2) ? cs1 : cs0, -m_new));
                        if constexpr (decltype(masked)::value) {
                            const int key = key0 + sb * 32 + mla_crow(i, g);
                            v = key <= lim ? v : 0.0f;
                        }
                        e[j] = v;
                        rs += v;
                    }
                    int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[0], e[1], 0, false);
                    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[2], e[3], w0, true);
                    int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[4], e[5], 0, false);
                    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[6], e[7], w1, true);
                    pw[2 * ch] = w0;
                    pw[2 * ch + 1] = w1;
                }
            };
            if (full) build_p(std::false_type{});
            else build_p(std::true_type{});
            l_run = l_run * alpha + rs;          // lane-partial; the lane pair is summed in the epilogue
        }
        // vmcnt(17) / vmcnt(0): V of tile t (8, the oldest) has landed; the next tile's 9 + 8 may fly -- the head comment has the count
        if (more) asm volatile("s_waitcnt vmcnt(17)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (active) {
            const unsigned char *vs = vring + slot * VTB;
            const v8i bv = {pw[0], pw[1], pw[2], pw[3], pw[4], pw[5], pw[6], pw[7]};
            auto v_operand = [&](int dt) {
                const v4u va = *reinterpret_cast<const v4u *>(vs + dt * 2048 + voff0);
                const v4u vb = *reinterpret_cast<const v4u *>(vs + dt * 2048 + voff1);
                return v8i{(int)va[0], (int)va[1], (int)va[2], (int)va[3], (int)vb[0], (int)vb[1], (int)vb[2], (int)vb[3]};
            };
            // O_j = O_j * alpha + T_j with T_j one tile's product from a zero accumulator, ONE output tile at a time: the product of tile j + 1
            // is issued, then tile j is folded under it, and the fence keeps the scheduler from raising more products (sixteen live T are
            // 256 registers).  O lives in the 256 accumulation registers, which the VALU cannot address: each element is read out, folded and
            // written back by name -- left to the allocator O moves into the ordinary registers and the loop spills (DESIGN 3.29 has the counts).
            // Every tile is folded: a second path that adds an unmoved tile through the MFMA's C operand brought the spills back.
            auto product = [&](int dt) {
                v16f acc;
#pragma unroll
                for (int i = 0; i < 16; i++) acc[i] = 0.0f;
                return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(v_operand(dt), bv, acc, 0, 0, 0, 0, 0, 0);     // (zero scale operands: the plain form)
            };
            v16f cur = product(0);
#pragma unroll
            for (int dt = 0; dt < NDT; dt++) {
                v16f nxt = cur;
                if (dt + 1 < NDT) nxt = product(dt + 1);
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    float ov, on;
                    asm("v_accvgpr_read_b32 %0, %1" : "=v"(ov) : "a"(o[dt][i]));
                    ov = __builtin_fmaf(ov, alpha, cur[i]);
                    asm("v_accvgpr_write_b32 %0, %1" : "=a"(on) : "v"(ov));
                    o[dt][i] = on;
                }
                __builtin_amdgcn_sched_barrier(0);
                cur = nxt;
            }
        }
        // (O stays in the accumulation registers between tiles)
#pragma unroll
        for (int dt = 0; dt < NDT; dt++) asm volatile("" : "+a"(o[dt]));
        ksc0 = ksn0;
        ksc1 = ksn1;
    }
    __syncthreads();          // every wave is past its last operand read: the ring is free for the output slabs

    // ---- epilogue: normalise, times the V scale, (cast,) transpose through LDS, store rows ----
    __builtin_amdgcn_s_setreg(kMlaModeFp16Ovfl, 0);
    const float l_tot = pair_sum(l_run);
    const float inv = l_tot > 0.0f ? __builtin_amdgcn_rcpf(l_tot) : 0.0f;
    unsigned char *obuf = smem + wave * (32 * DV * 2);       // 32 KiB per wave, 128 KiB of the ring's 136
    const float *vsc = p.v_scale + (long)b * DV;
    if constexpr (SPLIT) {
        // the FP32 partial O (1 / l) v_scale -- the expression below without the cast -- and log2(l) + m.  An FP32 row is 2048 bytes, the
        // wave's slab holds 32 rows of 1024: the row goes out in two halves of 256 channels, each transposed through the slab like the 16-bit
        // row below (a lane's four channels are ONE 16-byte chunk here; chunk q of 64 at q ^ (row & 15)) and stored as 32 pieces of 1 KiB.
        // Straight from the registers a store instruction would touch 64 separate 16-byte pieces 2 KiB apart.
        int n_e = lane & 31;                        // (the row formed again from the lane, opaquely: my_row kept across the loop was a spilled register)
        asm volatile("" : "+v"(n_e));
        if (g == 0 && row_ok) pp.lse_part[part_row0 + row0 + n_e] = l_tot > 0.0f ? __builtin_amdgcn_logf(l_tot) + m_run : -INFINITY;
        unsigned char *const pbase = reinterpret_cast<unsigned char *>(pp.o_part + part_row0 * DV);
#pragma unroll
        for (int half = 0; half < 2; half++) {
#pragma unroll
            for (int d8 = 0; d8 < NDT / 2; d8++) {
                const int dt = half * (NDT / 2) + d8;
#pragma unroll
                for (int r4 = 0; r4 < 4; r4++) {
                    const int d0 = dt * 32 + 8 * r4 + 4 * g;
                    const v4f sc4 = *reinterpret_cast<const v4f *>(vsc + d0);
                    v4f val;
#pragma unroll
                    for (int j = 0; j < 4; j++) val[j] = o[dt][4 * r4 + j] * inv * sc4[j];
                    const int q = (d0 - half * (DV / 2)) >> 2;      // 16-byte chunk of the half row's 64
                    *reinterpret_cast<v4f *>(obuf + n * 1024 + (q ^ (n & 15)) * 16) = val;
                }
            }
            // (the wave's own slab: its LDS operations execute in order -- the next half's writes behind these reads -- no workgroup barrier)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 4
            for (int r = 0; r < 32; r++) {
                const v4u val = *reinterpret_cast<const v4u *>(obuf + r * 1024 + (lane ^ (r & 15)) * 16);
                const int grow = row0 + r;
                if (grow < R) *reinterpret_cast<v4u *>(pbase + 4 * ((long)grow * DV) + half * 1024 + lane * 16) = val;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        return;
    }
    if (lse_b != nullptr && g == 0 && row_ok)       // (a row in front of key 0: l = 0, log2 gives -inf)
        lse_b[(long)my_head * Lq + my_pos] = l_tot > 0.0f ? __builtin_amdgcn_logf(l_tot) + m_run : -INFINITY;      // v_log_f32 is log2
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
            const int q8 = d0 >> 2;                             // 8-byte chunk of the 1024-byte row
            const int Q = (q8 >> 1) ^ (n & 15);                 // its 16-byte chunk of 64, the low four bits XOR-ed by the row
            *reinterpret_cast<v2u *>(obuf + n * (DV * 2) + Q * 16 + (q8 & 1) * 8) = pk;
        }
    }
    // (the wave's own slab: its writes and reads execute in order, no workgroup barrier)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 4
    for (int r = 0; r < 32; r++) {                              // 64 lanes of 16 bytes: one whole row per pass
        const v4u val = *reinterpret_cast<const v4u *>(obuf + r * (DV * 2) + (lane ^ (r & 15)) * 16);
        const int grow = row0 + r;
        if (grow < R) *reinterpret_cast<v4u *>(obase + 2 * ((long)grow * DV) + lane * 16) = val;
    }
}

}  // namespace sage
