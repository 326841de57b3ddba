// sage_split_exact.hip -- pass 1 of the exact split-KV route: the row maximum the attention kernel forms over each chunk of the key range.
//
// The exact split runs a call as S key-range chunks whose running maximum starts where the UNSPLIT call's would stand at the
// chunk's first tile, so that every P is rounded to e4m3 against the same maximum as in the unsplit call.  That starting value is the maximum
// of the chunk maxima in front of the chunk; this kernel computes them, with the attention kernel's own arithmetic:
//   * Q is quantised per thread group exactly as the fused-Q prologue does it (sage_attn_kernel.h, QF 1 / 2): same INT8 bits, same q scale;
//   * the raw INT32 scores come from the same v_mfma_i32_32x32x32_i8 products (exact), their maximum per (row, k scale group) is taken on the
//     integers and converted once: fma(max * 2^-26, ldexp(sm_scale_log2 * (q_scale * k_scale), 26), -log2(448)) -- the kernel's value for the
//     tile, bit for bit (the conversion is monotone, so the maximum commutes with it) -- and the maximum over the chunk's tiles and the two
//     lane halves of a row is exact;
//   * masking is the kernel's: key < Lk, and causal in global key coordinates (key <= row); a chunk with no visible key gives -inf.
// No softmax, no PV, no LDS: each wave reads its K fragments straight from global memory (the four waves of a workgroup share them through the
// cache), one tile ahead of the MFMAs.  Grid: one workgroup per (batch, kv head, chunk, query head of the group, 128-row query block).
// chunk_max_lens_kernel (below) is the same pass for the kv_lens family's split (num_splits=): a key length and a query offset per
// sample, one query block, chunks clipped to the sample's length.
// Replaces nothing in the reference (whose kernels do not split the key range).
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_quant_math.h"
#include "sage_chunk_max.h"
#include <climits>

namespace sage {

template <int D, int QDT, bool CAUSAL>
__global__ void __launch_bounds__(256, 2)
chunk_max_kernel(const ChunkMaxParams p)
{
    constexpr int KSTEPS = D / 32;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int n = lane & 31, g = lane >> 5;
    int idx = blockIdx.x;
    const int qblk = idx % p.nqblk;
    idx /= p.nqblk;
    const int gq = idx % p.group;
    idx /= p.group;
    const int c = idx % p.S;
    idx /= p.S;
    const int hk = idx % p.Hkv, b = idx / p.Hkv;
    const int h = hk * p.group + gq;
    const int row0 = qblk * BLKQ + wave * 32, my_row = row0 + n;
    if (row0 >= p.Lq) return;                   // (waves are independent: no LDS, no barrier)

    // ---- Q: the fused-Q prologue of sage_attn_kernel (QF 1 / 2), per-thread groups = rows r, r+8, r+16, r+24 of the wave, both halves ----
    // (one of THREE copies of this quantiser that must stay bit-equal: sage_attn_kernel.h's fused-Q prologue, this one, and cm_quant_q of sage_chunk_max.h)
    v4i qf[KSTEPS];
    float qsc;
    {
        const uint16_t *qrow = reinterpret_cast<const uint16_t *>(p.q) + (long)b * p.q_sb + (long)h * p.q_sh + (long)my_row * p.q_sl;
        const bool ok = my_row < p.Lq;
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

    // ---- the chunk's tiles (causal: those holding a key <= the wave's last row) ----
    const int t0 = c * p.tiles;
    int t1 = t0 + p.tiles;
    if (CAUSAL) {
        const int lim = (row0 + 31) / BLKK + 1;
        t1 = t1 < lim ? t1 : lim;
    }
    const int8_t *kb = p.k + (long)b * p.k_sb + (long)hk * p.k_sh;
    const float *ksb = p.k_scale + ((long)b * p.Hkv + hk) * p.nks;
    // lane (n, g) holds bytes 32 kk + 16 g .. + 15 of key rows 32 sb + n: the A operand of S^T = K Q^T (rows past Lk read the last one; masked below)
    auto load = [&](int t, v4i (&kf)[2][KSTEPS]) {
#pragma unroll
        for (int sb = 0; sb < 2; sb++) {
            int key = t * BLKK + sb * 32 + n;
            key = key < p.Lk ? key : p.Lk - 1;
            const int8_t *kr = kb + (long)key * p.k_sl + 16 * g;
#pragma unroll
            for (int kk = 0; kk < KSTEPS; kk++) kf[sb][kk] = *reinterpret_cast<const v4i *>(kr + 32 * kk);
        }
    };
    const int kmax = CAUSAL ? (my_row < p.Lk - 1 ? my_row : p.Lk - 1) : p.Lk - 1;      // the lane's last visible key: key < Lk, causal key <= row
    float mx = -INFINITY;
    v4i kc[2][KSTEPS], kn[2][KSTEPS];
    if (t0 < t1) load(t0, kc);
    for (int t = t0; t < t1; t++) {
        if (t + 1 < t1) load(t + 1, kn);
        v16i s[2];
#pragma unroll
        for (int sb = 0; sb < 2; sb++) {
#pragma unroll
            for (int i = 0; i < 16; i++) s[sb][i] = 0;
#pragma unroll
            for (int kk = 0; kk < KSTEPS; kk++) s[sb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(kc[sb][kk], qf[kk], s[sb], 0, 0, 0);
        }
        // per-thread k scale groups: 4 per 64 keys (token % 8 / 2); lane half g uses 2g (registers with i & 2 == 0) and 2g + 1
        const float s0 = ksb[4 * t + 2 * g], s1 = ksb[4 * t + 2 * g + 1];
        const float cs0 = __builtin_ldexpf(p.sm_scale_log2 * (qsc * s0), 26);
        const float cs1 = __builtin_ldexpf(p.sm_scale_log2 * (qsc * s1), 26);
        // (one select per score against the lane's last visible key, no branch: a wave-uniform `whole tile` branch around these selects was
        //  compiled into a write of INT_MIN over the MFMA result itself -- the first key of every masked tile was lost)
        int m0 = INT_MIN, m1 = INT_MIN;
#pragma unroll
        for (int sb = 0; sb < 2; sb++)
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int key = t * BLKK + sb * 32 + cm_crow(i, g);
                const int v = key <= kmax ? s[sb][i] : INT_MIN;
                if (i & 2) m1 = max(m1, v);
                else m0 = max(m0, v);
            }
        // (|score| <= 2^21: INT_MIN only where no key of the group is visible)
        if (m0 != INT_MIN) mx = fmaxf(mx, __builtin_fmaf(__builtin_ldexpf((float)m0, -26), cs0, -kFp8Offset));
        if (m1 != INT_MIN) mx = fmaxf(mx, __builtin_fmaf(__builtin_ldexpf((float)m1, -26), cs1, -kFp8Offset));
#pragma unroll
        for (int sb = 0; sb < 2; sb++)
#pragma unroll
            for (int kk = 0; kk < KSTEPS; kk++) kc[sb][kk] = kn[sb][kk];
    }
    mx = pair_max(mx);
    if (g == 0 && my_row < p.Lq)
        p.out[(((long)b * p.Hkv + hk) * p.S + c) * ((long)p.group * p.Lq) + (long)gq * p.Lq + my_row] = mx;
}

hipError_t launch_chunk_max(const ChunkMaxParams &p_in, hipStream_t stream)
{
    ChunkMaxParams p = p_in;
    p.nqblk = (p.Lq + BLKQ - 1) / BLKQ;
    const long nwg = (long)p.B * p.Hq * p.S * p.nqblk;
    if (nwg <= 0) return hipSuccess;
    if (nwg > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nwg), block(256);
#define SAGE_CM(D_, T_, C_) if (p.D == D_ && p.q_dtype == T_ && (p.causal != 0) == C_) { hipLaunchKernelGGL((chunk_max_kernel<D_, T_, C_>), grid, block, 0, stream, p); return hipGetLastError(); }
    SAGE_CM(128, DT_F16, false) SAGE_CM(128, DT_F16, true) SAGE_CM(128, DT_BF16, false) SAGE_CM(128, DT_BF16, true)
    SAGE_CM(64, DT_F16, false)  SAGE_CM(64, DT_F16, true)  SAGE_CM(64, DT_BF16, false)  SAGE_CM(64, DT_BF16, true)
#undef SAGE_CM
    return hipErrorInvalidValue;
}

// The same for the kv_lens family's split (ChunkMaxLensParams): sample b's keys end at len_b = clamp(kv_lens[b], 0, Lk) and, causal, row i sees
// key j iff j <= s_b + i with s_b = clamp(q_start[b], -Lq, Lk) -- the KVLEN / QSTART kernels' masks in global key coordinates.  Chunk c holds the
// tiles c * tiles .. + tiles - 1 that lie in front of ceil(len_b / 64) (and, causal, that hold a key the wave's last row sees); key rows, k scales
// and tiles from len_b on are never requested, and a chunk without a visible key writes -inf for every row.  A call has one query block.  With
// Lq <= 32 a wave serves one query head and a workgroup four heads of a GQA group, as the packed attention kernels (GPACK) map them -- one
// workgroup per query head would leave three waves without rows; else a workgroup is one query head, 32 rows per wave.
// Grid: B * Hkv * S * (Lq <= 32 ? ceil(group / 4) : group).
template <int D, int QDT, bool CAUSAL>
__global__ void __launch_bounds__(256, 2)
chunk_max_lens_kernel(const ChunkMaxLensParams p)
{
    constexpr int KSTEPS = D / 32;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int n = lane & 31, g = lane >> 5;
    const bool packed = p.Lq <= 32;
    const int per_kv = packed ? (p.group + 3) >> 2 : p.group;
    int idx = blockIdx.x;
    const int gi = idx % per_kv;
    idx /= per_kv;
    const int c = idx % p.S;
    idx /= p.S;
    const int hk = idx % p.Hkv, b = idx / p.Hkv;
    const int gq = packed ? 4 * gi + wave : gi;
    const int row0 = packed ? 0 : wave * 32, my_row = row0 + n;
    if (gq >= p.group || row0 >= p.Lq) return;  // (waves are independent: no LDS, no barrier)
    const int h = hk * p.group + gq;

    v4i qf[KSTEPS];
    float qsc;
    cm_quant_q<D, QDT>(reinterpret_cast<const uint16_t *>(p.q) + (long)b * p.q_sb + (long)h * p.q_sh + (long)my_row * p.q_sl, my_row < p.Lq, g, qf, qsc);

    // ---- the sample's length and offset, the chunk's tiles ----
    int len = p.kv_lens[b];
    len = len < 0 ? 0 : (len < p.Lk ? len : p.Lk);
    int s = 0;
    if (CAUSAL) {
        s = p.q_start != nullptr ? p.q_start[b] : 0;
        s = s < -p.Lq ? -p.Lq : (s < p.Lk ? s : p.Lk);
    }
    const int t0 = c * p.tiles;
    int t1 = t0 + p.tiles;
    const int nt = (len + BLKK - 1) / BLKK;
    t1 = t1 < nt ? t1 : nt;
    if (CAUSAL) {
        const int rlast = row0 + 31 < p.Lq ? row0 + 31 : p.Lq - 1;      // the wave's last row that exists
        const int vis = s + rlast;                                        // ... and the last key it sees
        const int lim = vis >= 0 ? vis / BLKK + 1 : 0;
        t1 = t1 < lim ? t1 : lim;
    }
    const int8_t *kb = p.k + (long)b * p.k_sb + (long)hk * p.k_sh;
    const float *ksb = p.k_scale + ((long)b * p.Hkv + hk) * p.nks;
    // (a tile that runs lies in front of ceil(len / 64), so len >= 1 here and rows from len on read row len - 1; masked below)
    auto load = [&](int t, v4i (&kf)[2][KSTEPS]) {
#pragma unroll
        for (int sb = 0; sb < 2; sb++) {
            int key = t * BLKK + sb * 32 + n;
            key = key < len ? key : len - 1;
            const int8_t *kr = kb + (long)key * p.k_sl + 16 * g;
#pragma unroll
            for (int kk = 0; kk < KSTEPS; kk++) kf[sb][kk] = *reinterpret_cast<const v4i *>(kr + 32 * kk);
        }
    };
    int kmax = len - 1;                         // the lane's last visible key (negative: none)
    if (CAUSAL) kmax = kmax < s + my_row ? kmax : s + my_row;
    float mx = -INFINITY;
    v4i kc[2][KSTEPS], kn[2][KSTEPS];
    if (t0 < t1) load(t0, kc);
    for (int t = t0; t < t1; t++) {
        if (t + 1 < t1) load(t + 1, kn);
        v16i sc[2];
#pragma unroll
        for (int sb = 0; sb < 2; sb++) {
#pragma unroll
            for (int i = 0; i < 16; i++) sc[sb][i] = 0;
#pragma unroll
            for (int kk = 0; kk < KSTEPS; kk++) sc[sb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(kc[sb][kk], qf[kk], sc[sb], 0, 0, 0);
        }
        const float s0 = ksb[4 * t + 2 * g], s1 = ksb[4 * t + 2 * g + 1];
        const float cs0 = __builtin_ldexpf(p.sm_scale_log2 * (qsc * s0), 26);
        const float cs1 = __builtin_ldexpf(p.sm_scale_log2 * (qsc * s1), 26);
        // (one select per score against the lane's last visible key, no branch: see chunk_max_kernel)
        int m0 = INT_MIN, m1 = INT_MIN;
#pragma unroll
        for (int sb = 0; sb < 2; sb++)
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int key = t * BLKK + sb * 32 + cm_crow(i, g);
                const int v = key <= kmax ? sc[sb][i] : INT_MIN;
                if (i & 2) m1 = max(m1, v);
                else m0 = max(m0, v);
            }
        if (m0 != INT_MIN) mx = fmaxf(mx, __builtin_fmaf(__builtin_ldexpf((float)m0, -26), cs0, -kFp8Offset));
        if (m1 != INT_MIN) mx = fmaxf(mx, __builtin_fmaf(__builtin_ldexpf((float)m1, -26), cs1, -kFp8Offset));
#pragma unroll
        for (int sb = 0; sb < 2; sb++)
#pragma unroll
            for (int kk = 0; kk < KSTEPS; kk++) kc[sb][kk] = kn[sb][kk];
    }
    mx = pair_max(mx);
    if (g == 0 && my_row < p.Lq)
        p.out[(((long)b * p.Hkv + hk) * p.S + c) * ((long)p.group * p.Lq) + (long)gq * p.Lq + my_row] = mx;
}

hipError_t launch_chunk_max_lens(const ChunkMaxLensParams &p, hipStream_t stream)
{
    if (p.Lq > BLKQ || p.Lq <= 0 || p.S <= 0 || p.tiles <= 0 || p.kv_lens == nullptr) return hipErrorInvalidValue;
    const long per_kv = p.Lq <= 32 ? (p.group + 3) / 4 : p.group;
    const long nwg = (long)p.B * p.Hkv * p.S * per_kv;
    if (nwg <= 0) return hipSuccess;
    if (nwg > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nwg), block(256);
#define SAGE_CML(D_, T_, C_) if (p.D == D_ && p.q_dtype == T_ && (p.causal != 0) == C_) { hipLaunchKernelGGL((chunk_max_lens_kernel<D_, T_, C_>), grid, block, 0, stream, p); return hipGetLastError(); }
    SAGE_CML(128, DT_F16, false) SAGE_CML(128, DT_F16, true) SAGE_CML(128, DT_BF16, false) SAGE_CML(128, DT_BF16, true)
    SAGE_CML(64, DT_F16, false)  SAGE_CML(64, DT_F16, true)  SAGE_CML(64, DT_BF16, false)  SAGE_CML(64, DT_BF16, true)
#undef SAGE_CML
    return hipErrorInvalidValue;
}

}  // namespace sage
