// sage_mla_attn.hip -- fused INT8-QK^T / online-softmax / FP8-PV attention for the ABSORBED multi-head-latent-attention decode shape on gfx950:
// every query head of a sample reads one shared latent row of 576 channels per token, and V is the first 512 channels of that row
// (include/sage_mla_gfx950.h).  A kernel of its own beside the D = 64 / 128 family, the head_dim = 256 kernel and the 192 / 128
// one: their arithmetic, another work item, register file and LDS plan.
//
//  * work item = 128 rows of the flattened [Lq * Hq] row space of ONE sample against the sample's whole latent: row r is position r / Hq, head
//    r % Hq.  Four waves of 32 rows, grid B x ceil(Lq * Hq / 128).  128 rows per K byte is the point of the shape: a sample's heads are not
//    split over workgroups (DESIGN 3.29 has the estimate).
//  * the family's swapped products: S^T = K Q^T on v_mfma_i32_32x32x32_i8 (A = K rows from LDS, B = the wave's Q fragments, EIGHTEEN k-steps
//    per 32 keys, two sub-tiles per 64-key tile), so that a lane holds 16 keys of ONE query row -- its Q scale, m, l and key limit are one
//    value each per lane -- and the converted P is already the B operand of O^T = V^T P^T on v_mfma_f32_32x32x64_f8f6f4 (A = 32 channels x 64
//    positions of the V image, SIXTEEN output tiles per 64 keys).
//  * Q: INT8 with one scale per query row.  The reference's per-thread groups are rows r, r + 8, r + 16, r + 24 of one head
//    (quant_per_thread.py:21-52); with Lq <= 8 a decode row is alone in its group, and this kernel keeps that definition for every Lq: its
//    flattened rows mix heads in a wave, and a scale shared across heads would be an invention.
//  * registers: O^T is 16 x 16 = 256 FP32 registers per lane, the Q fragments 72, one tile's scores 32, P 8, a two-level product 16.  Built
//    under __launch_bounds__(256, 1): one wave per SIMD on purpose, the whole 512-register file to it (DESIGN 3.29 has the compiler's counts).
//    O fills the 256 accumulation registers, everything else the ordinary ones.  The sixteen PV products of a tile are consumed ONE output
//    tile at a time, O_j = O_j * alpha + T_j, with the next tile's product the only other one in flight: sixteen live T would be 256 more
//    registers, so the loop is fenced per output tile, and O is read out of and written back to its registers by name.
//  * LDS: 136 KiB of dynamic shared memory -- a two-slot ring of 36-KiB K tiles and a two-slot ring of 32-KiB V tiles; one workgroup per CU.
//    Both images are stored by the pre-pass in their in-LDS order (sage_mla.h), so a K tile is 36 lane-linear 1-KiB LDS-DMA pieces, NINE per
//    wave, a V tile 32, EIGHT per wave, and every MFMA operand read is a ds_read_b128 in the panel format whose bank argument is
//    sage_qk192.h's.  Tile t + 1 is requested behind the barrier at the top of tile t: the K slot it lands in was read by tile t - 1's QK^T,
//    the V slot by tile t - 1's PV, both behind that barrier for every wave.
//  * the counted waits.  The counter retires in order and nothing else of the loop is a vector memory operation (the four K scales of a tile
//    come by one wave-uniform scalar load, one tile ahead, the lane's two chosen by a select).  At the top of tile t the wave's counted
//    instructions are, oldest first, K of t (9) and V of t (8) -- requested in the prologue, or behind the top barrier of tile t - 1, whose PV
//    wait left exactly these seventeen: vmcnt(8) means K has landed and V may still fly.  In front of PV they are V of t (8) and, if there is
//    a next tile, its K (9) and V (8) just requested: vmcnt(17) means V of t has landed with the whole next tile in flight; on the last tile
//    nothing younger exists, vmcnt(0).  Each wait is followed by a raw barrier: everybody's pieces.  The prologue's request of tile 0 is
//    unconditional for every item that reaches it; an item with no visible key leaves before it (a workgroup-uniform test), writing zeros
//    and -inf.
//  * score conversion: v_cvt_f32_i32.  |s| reaches 127 * 127 * 576 = 9 290 304, below the 2^24 the conversion takes exactly; the accumulators
//    start from zero.
//  * mask: the decode one, bottom-right: the row at position i sees key j iff j <= kv_len - Lq + i.  Applied per score in front of the row
//    maximum on tiles that contain some row's limit; tiles wholly in front of every limit of the wave take the raw-integer maximum; a wave
//    whose rows all lie in front of a tile's first key skips the arithmetic and keeps its barriers.
//  * epilogue: O / l times the V scale, cast, transposed through the wave's own 32-KiB slab of the (free) ring -- 32 rows of 1024 bytes, the
//    16-byte chunks XOR-ed by row & 15 -- and stored as whole 1024-byte rows.
#include "../../include/sage_mla_gfx950.h"
#include "sage_mla.h"
#include "sage_host_checks.h"
#include "sage_quant_math.h"

#include <atomic>
#include <climits>
#include <type_traits>

namespace sage {

// hwreg(HW_REG_MODE, 23, 1): MODE.FP16_OVFL -- conversions saturate to the largest finite value
constexpr int kMlaModeFp16Ovfl = 1 | (23 << 6) | (0 << 11);

// c/d register r of a 32x32 MFMA tile -> row index inside the tile (lane half g = lane >> 5)
__device__ __forceinline__ int mla_crow(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }

template <int DT>
__global__ void __launch_bounds__(256, 1) mla_decode_kernel(const MlaAttnParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int DQK = MLA_DQK, DV = MLA_DV, KSTEPS = DQK / 32, NDT = DV / 32, KTB = MLA_K_TILE_BYTES, VTB = MLA_V_TILE_BYTES;
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int n = lane & 31, g = lane >> 5;

    // ---- work item: (sample, 128-row block of its [Lq * Hq] rows) ----
    const int b = (int)blockIdx.x / p.nblk, blk = (int)blockIdx.x % p.nblk;
    const int R = p.rows, Hq = p.Hq, Lq = p.Lq;
    const int kvlen = mla_kv_len(p.kv_lens, b, p.Lk);
    const int shift = kvlen - Lq;                                       // the row at position i sees keys j <= i + shift
    const int blk_last = (blk * BLKQ + BLKQ < R ? blk * BLKQ + BLKQ : R) - 1;          // the item's last valid row
    const int kend = blk_last / Hq + shift + 1;                         // its limit + 1; at most kvlen
    unsigned char *const obase = reinterpret_cast<unsigned char *>(p.o) + 2 * ((long)b * R * DV);
    float *const lse_b = p.lse != nullptr ? p.lse + (long)b * Hq * Lq : nullptr;

    if (kend <= 0) {            // (workgroup-uniform) no row of the item sees a key: o = +0, lse = -inf, and nothing was requested
        const int nrow = blk_last - blk * BLKQ + 1;
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

    const int n_tiles = (kend + BLKK - 1) / BLKK;       // >= 1, <= the tiles the pre-pass wrote for the sample
    const unsigned char *kimg = p.k_img + (long)b * p.ntile * KTB;
    const unsigned char *vimg = p.v_img + (long)b * p.ntile * VTB;
    typedef const __attribute__((address_space(4))) float *cfloat_p;       // K scales by scalar loads: a VGPR load would join the DMA's counter
    const cfloat_p ks_c = (cfloat_p)(p.k_scale + (long)b * p.ntile * 4);

    // a tile = PIECES-per-wave x four waves of 1-KiB pieces (K: 9, V: 8); source and destination are lane-linear
    auto issue_tile = [&](const unsigned char *src_tile, unsigned char *slot, auto pieces_tag) {
        constexpr int PIECES = decltype(pieces_tag)::value;
        const unsigned char *src = src_tile + wave * (PIECES * 1024) + lane * 16;
#pragma unroll
        for (int i = 0; i < PIECES; i++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + i * 1024),
                                             (__attribute__((address_space(3))) void *)(slot + wave * (PIECES * 1024) + i * 1024), 16, 0, 0);
    };
    using KPieces = std::integral_constant<int, KTB / 4096>;     // 9
    using VPieces = std::integral_constant<int, VTB / 4096>;     // 8
    unsigned char *const kring = smem, *const vring = smem + 2 * KTB;
    issue_tile(kimg, kring, KPieces{});
    issue_tile(vimg, vring, VPieces{});

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

    // ---- Q: the lane's 16 channels of every k-step of its row, INT8 with one scale per row, into the B operands ----
    v4i qf[KSTEPS];
    float qsc;
    {
        const uint16_t *qrow = reinterpret_cast<const uint16_t *>(p.q) + (long)b * p.q_sb + (long)my_pos * p.q_sl + (long)my_head * p.q_sh;
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

    v16f o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; dt++)
#pragma unroll
        for (int i = 0; i < 16; i++) o[dt][i] = 0.0f;
    float m_run = kNegBig, l_run = 0.0f;

    // the lane's two K scales of a tile: keys of registers with (i & 2) == 0 / != 0 lie in groups 2 g / 2 g + 1 of quant_per_thread.py:75-83
    auto k_scales = [&](int t, float &s0, float &s1) {
        const float a0 = ks_c[4 * t], a1 = ks_c[4 * t + 1], a2 = ks_c[4 * t + 2], a3 = ks_c[4 * t + 3];
        s0 = g ? a2 : a0;
        s1 = g ? a3 : a1;
    };
    float ksc0, ksc1;
    k_scales(0, ksc0, ksc1);

    // the lane's operand offsets inside a slot: K row n of sub-tile 0 (sub-tile 1 is 32 rows = 2048 bytes on, the same swizzle), chunk
    // (2 kk + g) & 3 = 2 (kk & 1) + g of panel kk >> 1; V channel n of output tile 0 (tile dt is 32 channels = 2048 bytes on)
    const int koff0 = n * 64 + swz_chunk<64>(n, g) * 16, koff1 = n * 64 + swz_chunk<64>(n, 2 + g) * 16;
    const int voff0 = n * 64 + swz_chunk<64>(n, 2 * g) * 16, voff1 = n * 64 + swz_chunk<64>(n, 2 * g + 1) * 16;

    for (int t = 0; t < n_tiles; t++) {
        const int slot = t & 1;
        const bool more = t + 1 < n_tiles;
        // vmcnt(8): K of tile t (9, the older) has landed, V of tile t (8) may still fly -- the head comment has the count
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        float ksn0 = 0.0f, ksn1 = 0.0f;
        if (more) {
            issue_tile(kimg + (long)(t + 1) * KTB, kring + (slot ^ 1) * KTB, KPieces{});
            issue_tile(vimg + (long)(t + 1) * VTB, vring + (slot ^ 1) * VTB, VPieces{});
            k_scales(t + 1, ksn0, ksn1);
        }
        const int key0 = t * BLKK;
        const bool active = wave_ok && key0 <= lim_hi;          // (wave-uniform) some row of the wave sees a key of the tile
        int pw[8];                                              // P of the tile: 32 e4m3 per lane, the B operand of PV
        float alpha = 1.0f;
        if (active) {
            const unsigned char *ks = kring + slot * KTB;
            // ---- S^T = K Q^T, two sub-tiles of 32 keys, eighteen k-steps each: k-step kk reads chunk 2 kk + g of the row's 36 ----
            v16i s[2];
#pragma unroll
            for (int sb = 0; sb < 2; sb++) {
#pragma unroll
                for (int i = 0; i < 16; i++) s[sb][i] = 0;
#pragma unroll
                for (int kk = 0; kk < KSTEPS; kk++) {
                    const v4i a = *reinterpret_cast<const v4i *>(ks + (kk >> 1) * MLA_PANEL_BYTES + sb * 2048 + ((kk & 1) ? koff1 : koff0));
                    s[sb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, qf[kk], s[sb], 0, 0, 0);
                }
            }
            // the reference's order: sm_scale log2(e) * (q_scale * k_scale)  (qk_int_sv_f8_cuda_sm89.cuh:263-266)
            const float cs0 = p.sm_scale_log2 * (qsc * ksc0), cs1 = p.sm_scale_log2 * (qsc * ksc1);
            const bool full = key0 + BLKK - 1 <= lim_lo;        // (wave-uniform) every row of the wave sees the whole tile
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
                        const int key = key0 + sb * 32 + mla_crow(i, g);
                        mx = fmaxf(mx, key <= lim ? __builtin_fmaf((float)s[sb][i], (i & 2) ? cs1 : cs0, -kFp8Offset) : -INFINITY);
                    }
            }
            // (a row that has seen no key yet keeps m_run = kNegBig: alpha = exp2(0) = 1, its exp2 below overflows to +inf and the mask turns
            // it into 0 BEFORE the row sum; `full` is never true for such a row's wave)
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
                    pw[2 * c] = w0;
                    pw[2 * c + 1] = w1;
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

    // ---- epilogue: normalise, times the V scale, cast, transpose through LDS, store rows ----
    __builtin_amdgcn_s_setreg(kMlaModeFp16Ovfl, 0);
    const float l_tot = pair_sum(l_run);
    const float inv = l_tot > 0.0f ? __builtin_amdgcn_rcpf(l_tot) : 0.0f;
    if (lse_b != nullptr && g == 0 && row_ok)       // (a row in front of key 0: l = 0, log2 gives -inf)
        lse_b[(long)my_head * Lq + my_pos] = l_tot > 0.0f ? __builtin_amdgcn_logf(l_tot) + m_run : -INFINITY;      // v_log_f32 is log2
    unsigned char *obuf = smem + wave * (32 * DV * 2);       // 32 KiB per wave, 128 KiB of the ring's 136
    const float *vsc = p.v_scale + (long)b * DV;
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

hipError_t launch_mla_attn(const MlaAttnParams &p, int dtype, hipStream_t stream)
{
    const dim3 grid((unsigned)((long)p.B * p.nblk)), block(256);
    if (dtype == DT_F16) hipLaunchKernelGGL(mla_decode_kernel<DT_F16>, grid, block, MLA_LDS_BYTES, stream, p);
    else hipLaunchKernelGGL(mla_decode_kernel<DT_BF16>, grid, block, MLA_LDS_BYTES, stream, p);
    return hipGetLastError();
}

// 136 KiB of dynamic shared memory is above the 64 KiB a kernel gets unasked: the attribute is set once per process and device (lock-free: a
// race repeats the idempotent calls), and a device that offers less is refused.  0 = ready; otherwise the message is set.
static int mla_lds_ready(const char *e)
{
    static std::atomic<unsigned long long> done{0};         // bit per device ordinal (mod 64)
    int dev = -1, lds = 0, optin = 0;
    hipError_t err = hipGetDevice(&dev);
    if (err != hipSuccess || dev < 0) return set_last_error(SAGE_EINVAL, "%s: no current device: %s", e, hipGetErrorString(err));
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_relaxed) & bit) return 0;
    err = hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    if (err != hipSuccess) return set_last_error(SAGE_EINVAL, "%s: cannot read the device's LDS size: %s", e, hipGetErrorString(err));
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) (void)hipGetLastError();
    if (optin > lds) lds = optin;
    if (lds < MLA_LDS_BYTES)
        return set_last_error(SAGE_EINVAL, "%s: the device offers %d bytes of LDS per workgroup, the kernel needs %d", e, lds, MLA_LDS_BYTES);
    err = hipFuncSetAttribute(reinterpret_cast<const void *>(&mla_decode_kernel<DT_F16>), hipFuncAttributeMaxDynamicSharedMemorySize, MLA_LDS_BYTES);
    if (err == hipSuccess)
        err = hipFuncSetAttribute(reinterpret_cast<const void *>(&mla_decode_kernel<DT_BF16>), hipFuncAttributeMaxDynamicSharedMemorySize, MLA_LDS_BYTES);
    if (err != hipSuccess)
        return set_last_error(SAGE_EINVAL, "%s: cannot raise the kernel's dynamic LDS to %d bytes: %s", e, MLA_LDS_BYTES, hipGetErrorString(err));
    done.fetch_or(bit, std::memory_order_relaxed);
    return 0;
}

}  // namespace sage

extern "C" {

using namespace sage;

SAGE_MLA_API int sage_mla_abi_version(void) { return SAGE_MLA_ABI_VERSION; }

SAGE_MLA_API int sage_mla_attn(const void *q, const void *k_image, const void *v_image, const float *k_scale, const float *v_scale,
                               const int32_t *kv_lens, void *o, float *lse, int B, int Lq, int Hq, int Lk, int width_qk, int width_v,
                               int64_t q_sb, int64_t q_sl, int64_t q_sh, float sm_scale, int dtype, void *stream)
{
    const char *const e = "sage_mla_attn";
    SAGE_REQUIRE(width_qk == MLA_DQK && width_v == MLA_DV,
                 "%s: width_qk must be 576 and width_v 512 (got %d and %d); call sage_qk192_attn for 192 / 128, sage_hd256_attn for one head_dim up to 256, sage_attn_fused_q_pv_f8 for 64 / 128",
                 e, width_qk, width_v);
    SAGE_REQUIRE(dtype == DT_F16 || dtype == DT_BF16, "%s: dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got %d)", e, dtype);
    SAGE_REQUIRE(B >= 1 && Lq >= 1 && Hq >= 1 && Lk >= 1, "%s: empty problem (B %d, Lq %d, Hq %d, Lk %d)", e, B, Lq, Hq, Lk);
    SAGE_REQUIRE(q && k_image && v_image && k_scale && v_scale && o, "%s: null pointer (only kv_lens and lse may be null)", e);
    SAGE_REQUIRE(aligned16_strides(q, 8, q_sb, q_sl, q_sh) && q_sb >= 0 && q_sl >= 0 && q_sh >= 0 && aligned16(o),
                 "%s: q and o must be 16-byte aligned, q with non-negative strides in multiples of 8 elements", e);
    SAGE_REQUIRE(aligned16(k_image) && aligned16(v_image) && aligned16(v_scale) && aligned4(k_scale) && aligned4(kv_lens) && aligned4(lse),
                 "%s: the images and v_scale must be 16-byte aligned, k_scale, kv_lens and lse 4-byte", e);
    const int64_t rows = (int64_t)Lq * Hq, nblk = (rows + BLKQ - 1) / BLKQ;
    SAGE_REQUIRE(rows < ((int64_t)1 << 31) && B * nblk < ((int64_t)1 << 31), "%s: Lq * Hq and B * ceil(Lq * Hq / 128) must be below 2^31", e);
    if (mla_lds_ready(e) != 0) return SAGE_EINVAL;
    MlaAttnParams p{};
    p.q = q; p.k_img = static_cast<const unsigned char *>(k_image); p.v_img = static_cast<const unsigned char *>(v_image);
    p.k_scale = k_scale; p.v_scale = v_scale; p.kv_lens = kv_lens; p.o = o; p.lse = lse;
    p.q_sb = q_sb; p.q_sl = q_sl; p.q_sh = q_sh;
    p.B = B; p.Lq = Lq; p.Hq = Hq; p.Lk = Lk; p.rows = (int)rows; p.nblk = (int)nblk; p.ntile = (Lk + BLKK - 1) / BLKK;
    p.sm_scale_log2 = sm_scale * 1.44269504088896340736f;      // in FP32, as the reference's kernel forms it (qk_int_sv_f8_cuda_sm89.cuh:90)
    const hipError_t err = launch_mla_attn(p, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
