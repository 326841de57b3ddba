// sage_qk192_attn.hip -- fused INT8-QK^T / online-softmax / FP8-PV attention for 192-wide Q / K rows against 128-wide V rows on gfx950: the
// multi-head-latent-attention prefill shape (include/sage_qk192_gfx950.h).  A kernel of its own beside the D = 64 / 128
// family (sage_attn_kernel.h) and the head_dim = 256 kernel (sage_hd256_attn.hip): their arithmetic, another register file and LDS plan.
//
//  * work item = 128 query rows of one query head, four waves of 32 rows, and the family's swapped products: S^T = K Q^T on
//    v_mfma_i32_32x32x32_i8 (A = K rows from LDS, B = the wave's Q fragments, SIX k-steps per 32 keys), so that a lane holds 16 keys of ONE
//    query row and the converted P is already the B operand of O^T = V^T P^T on v_mfma_f32_32x32x64_f8f6f4 (A = 32 channels x 64 positions
//    of the V image, FOUR output tiles per 64 keys).
//  * registers: O^T is 4 x 16 = 64 FP32 registers per lane, the INT8 Q fragments 24, one tile's scores 32, P 8, and the two-level products
//    of a tile 16 each.  Built under __launch_bounds__(256, 2): two waves per SIMD, two workgroups per CU (DESIGN 3.27 has the compiler's
//    counts).
//  * LDS: 40 KiB -- a two-slot ring of 12-KiB K tiles and a two-slot ring of 8-KiB V images, so two workgroups take 80 of a CU's 160 KiB.
//    Two slots, not three: the load of tile t + 1 is requested behind the barrier at the top of tile t and has that whole tile (QK^T, softmax,
//    PV) to land, and the second workgroup of the CU computes while this one waits; a third slot would only pay if a barrier per tile could
//    go with it, and that is not measured.  Both images are stored by the pre-pass in their in-LDS order (sage_qk192.h), so a K tile is twelve
//    lane-linear 1-KiB LDS-DMA pieces, THREE per wave, a V tile eight, TWO per wave, and every MFMA operand read is a conflict-free
//    ds_read_b128.  The K slot that tile t + 1 lands in was read by tile t - 1's QK^T, the V slot by tile t - 1's PV, both behind the top
//    barrier of tile t for every wave.  The waits are counted -- derived at each -- and the barriers raw.
//  * score conversion: v_cvt_f32_i32.  |s| reaches 127 * 127 * 192 = 3 096 768: above the 2^21 up to which the family's mid-binade start
//    value is exact, below the 2^24 the conversion instruction takes exactly.
//  * softmax as the family's general tile: log2 domain, exp2(fma(s, c, -m)), the mask in front of the row maximum, P saturated to e4m3
//    (MODE.FP16_OVFL), the row sum over the unrounded P, O = O * alpha + T with T one tile's product from a zero accumulator.  A whole
//    unmasked tile takes its row maxima on the raw integers (c >= 0), and a tile in which no row maximum of the wave moved adds its product to
//    O through the MFMA's FP32 C operand.
//  * causal launches run the heaviest query blocks first (a reversed block index), the query heads of a GQA group next to each other.
//  * epilogue: O / l times the V scale, cast, transposed through the wave's own 8-KiB slab of the (free) ring, stored as whole 256-byte rows.
#include "../../include/sage_qk192_gfx950.h"
#include "sage_qk192.h"
#include "sage_host_checks.h"
#include "sage_quant_math.h"

#include <climits>
#include <type_traits>

namespace sage {

// hwreg(HW_REG_MODE, 23, 1): MODE.FP16_OVFL -- conversions saturate to the largest finite value
constexpr int kQk192ModeFp16Ovfl = 1 | (23 << 6) | (0 << 11);

// c/d register r of a 32x32 MFMA tile -> row index inside the tile (lane half g = lane >> 5)
__device__ __forceinline__ int qk192_crow(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }

template <bool CAUSAL, int DT>
__global__ void __launch_bounds__(256, 2) qk192_attn_kernel(const Qk192AttnParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int DQK = QK192_DQK, DV = QK192_DV, KSTEPS = DQK / 32, NDT = DV / 32, KTB = QK192_K_TILE_BYTES, VTB = QK192_V_TILE_BYTES;
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int n = lane & 31, g = lane >> 5;
    __builtin_amdgcn_s_setreg(kQk192ModeFp16Ovfl, 1);

    // ---- work item: query head fastest (a GQA group streams one kv head's images together), the heaviest causal blocks first ----
    const int bid = blockIdx.x;
    const int h = bid % p.Hq, rest = bid / p.Hq;
    const int b = rest % p.B, qr = rest / p.B;
    const int qblk = CAUSAL ? p.nqblk - 1 - qr : qr;
    const int hk = h / p.group;
    const int Lk = p.Lk, Lq = p.Lq;
    const int row0 = qblk * BLKQ + wave * 32;           // the wave's first query row
    const int my_row = row0 + n;
    const int kend = CAUSAL ? (Lk < qblk * BLKQ + BLKQ ? Lk : qblk * BLKQ + BLKQ) : Lk;
    const int n_tiles = (kend + BLKK - 1) / BLKK;       // >= 1, <= ntile
    const unsigned char *kimg = p.k_img + ((long)b * p.Hkv + hk) * p.ntile * KTB;
    const unsigned char *vimg = p.v_img + ((long)b * p.Hkv + hk) * p.ntile * VTB;
    typedef const __attribute__((address_space(4))) float *cfloat_p;       // K scales by scalar loads: a VGPR load would join the DMA's counter
    const cfloat_p ks_c = (cfloat_p)(p.k_scale + ((long)b * p.Hkv + hk) * p.ntile * 4);

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
        const uint16_t *qrow = reinterpret_cast<const uint16_t *>(p.q) + (long)b * p.q_sb + (long)h * p.q_sh + (long)my_row * p.q_sl;
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
        const bool active = !CAUSAL || key0 <= row0 + 31;       // (wave-uniform) some row of the wave sees a key of the tile
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
            const float cs0 = p.sm_scale_log2 * (qsc * ksc0), cs1 = p.sm_scale_log2 * (qsc * ksc1);
            const bool full = (key0 + BLKK <= Lk) && (!CAUSAL || key0 + BLKK - 1 <= row0);
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
                        const bool ok = key < Lk && (!CAUSAL || key <= my_row);
                        mx = fmaxf(mx, ok ? __builtin_fmaf((float)s[sb][i], (i & 2) ? cs1 : cs0, -kFp8Offset) : -INFINITY);
                    }
            }
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
                            v = (key < Lk && (!CAUSAL || key <= my_row)) ? v : 0.0f;
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
    if (p.lse != nullptr && g == 0 && my_row < Lq)
        p.lse[((long)b * p.Hq + h) * (long)Lq + my_row] = __builtin_amdgcn_logf(l_tot) + m_run;      // v_log_f32 is log2
    unsigned char *obuf = smem + wave * (32 * DV * 2);       // 8 KiB per wave, 32 KiB of the ring's 40
    const float *vsc = p.v_scale + ((long)b * p.Hkv + hk) * DV;
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
    unsigned char *obase = reinterpret_cast<unsigned char *>(p.o) + 2 * ((long)b * p.o_sb + (long)h * p.o_sh);
#pragma unroll
    for (int pass = 0; pass < 8; pass++) {                      // 16 lanes of 16 bytes per row, four rows per pass
        const int r = 4 * pass + (lane >> 4), Q = lane & 15;
        const v4u val = *reinterpret_cast<const v4u *>(obuf + r * (DV * 2) + (Q ^ (r & 15)) * 16);
        const int grow = row0 + r;
        if (grow < Lq) *reinterpret_cast<v4u *>(obase + 2 * ((long)grow * p.o_sl) + Q * 16) = val;
    }
}

hipError_t launch_qk192_attn(const Qk192AttnParams &p, bool causal, int dtype, hipStream_t stream)
{
    const dim3 grid((unsigned)((long)p.B * p.Hq * p.nqblk)), block(256);
#define SAGE_QK192_LAUNCH(C, T) hipLaunchKernelGGL((qk192_attn_kernel<C, T>), grid, block, QK192_LDS_BYTES, stream, p)
    if (causal) { if (dtype == DT_F16) SAGE_QK192_LAUNCH(true, DT_F16); else SAGE_QK192_LAUNCH(true, DT_BF16); }
    else { if (dtype == DT_F16) SAGE_QK192_LAUNCH(false, DT_F16); else SAGE_QK192_LAUNCH(false, DT_BF16); }
#undef SAGE_QK192_LAUNCH
    return hipGetLastError();
}

static bool qk192_rows_ok(const void *ptr, int64_t sb, int64_t sh, int64_t sl, int width)
{
    return aligned16_strides(ptr, 8, sb, sh, sl) && sb >= 0 && sh >= 0 && sl >= width;
}

}  // namespace sage

extern "C" {

using namespace sage;

SAGE_QK192_API int sage_qk192_abi_version(void) { return SAGE_QK192_ABI_VERSION; }

SAGE_QK192_API int sage_qk192_attn(const void *q, const void *k_image, const void *v_image, const float *k_scale, const float *v_scale,
                                   void *o, float *lse, int B, int Hq, int Hkv, int Lq, int Lk, int head_dim_qk, int head_dim_v,
                                   int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                   int is_causal, float sm_scale, int dtype, void *stream)
{
    const char *const e = "sage_qk192_attn";
    SAGE_REQUIRE(head_dim_qk == QK192_DQK && head_dim_v == QK192_DV,
                 "%s: head_dim_qk must be 192 and head_dim_v 128 (got %d and %d); zero-pad 129 .. 191 / 1 .. 127, and call sage_hd256_attn for wider rows, sage_attn_fused_q_pv_f8 for 64 / 128",
                 e, head_dim_qk, head_dim_v);
    SAGE_REQUIRE(dtype == DT_F16 || dtype == DT_BF16, "%s: dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got %d)", e, dtype);
    SAGE_REQUIRE(B >= 1 && Hq >= 1 && Hkv >= 1 && Lq >= 1 && Lk >= 1, "%s: empty problem (B %d, Hq %d, Hkv %d, Lq %d, Lk %d)", e, B, Hq, Hkv, Lq, Lk);
    SAGE_REQUIRE(Hq % Hkv == 0, "%s: Hq (%d) must be a multiple of Hkv (%d)", e, Hq, Hkv);
    SAGE_REQUIRE(q && k_image && v_image && k_scale && v_scale && o, "%s: null pointer (only lse may be null)", e);
    SAGE_REQUIRE(qk192_rows_ok(q, q_sb, q_sh, q_sl, QK192_DQK) && qk192_rows_ok(o, o_sb, o_sh, o_sl, QK192_DV),
                 "%s: q and o must be 16-byte aligned with non-negative strides in multiples of 8 elements and a token stride of at least 192 (q) / 128 (o)", e);
    SAGE_REQUIRE(aligned16(k_image) && aligned16(v_image) && aligned16(v_scale) && aligned4(k_scale) && aligned4(lse),
                 "%s: the images and v_scale must be 16-byte aligned, k_scale and lse 4-byte", e);
    const int nqblk = (Lq + BLKQ - 1) / BLKQ;
    SAGE_REQUIRE((int64_t)B * Hq * nqblk < ((int64_t)1 << 31), "%s: B * Hq * ceil(Lq / 128) must be below 2^31", e);
    Qk192AttnParams p{};
    p.q = q; p.k_img = static_cast<const unsigned char *>(k_image); p.v_img = static_cast<const unsigned char *>(v_image);
    p.k_scale = k_scale; p.v_scale = v_scale; p.o = o; p.lse = lse;
    p.q_sb = q_sb; p.q_sh = q_sh; p.q_sl = q_sl; p.o_sb = o_sb; p.o_sh = o_sh; p.o_sl = o_sl;
    p.B = B; p.Hq = Hq; p.Hkv = Hkv; p.Lq = Lq; p.Lk = Lk; p.nqblk = nqblk; p.ntile = (Lk + BLKK - 1) / BLKK; p.group = Hq / Hkv;
    p.sm_scale_log2 = sm_scale * 1.44269504088896340736f;      // in FP32, as the reference's kernel forms it (qk_int_sv_f8_cuda_sm89.cuh:90)
    const hipError_t err = launch_qk192_attn(p, is_causal != 0, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
