// sage_merge.hip -- merge of two partial attention states by their log-sum-exp (HBM-bound, elementwise).
//
// The reference exposes `return_lse` (core.py:782-786, 823-826) as its only long-context hook: sequence-parallel
// callers (ring attention, example/parallel_sageattn_cogvideo.py via xfuser) run attention against one K/V shard at
// a time and combine the partial outputs with
//     m = max(lse_a, lse_b);  w_a = e^(lse_a - m);  w_b = e^(lse_b - m)
//     o = (o_a w_a + o_b w_b) / (w_a + w_b);        lse = m + log(w_a + w_b)
// This kernel keeps the running state (o_acc, lse_acc) in FP32 across the steps of the ring so the output is
// rounded to fp16/bf16 exactly once, at the last step.  One thread owns 8 channels of one (batch, head, row):
// 32 B of accumulator + 16 B of new output in, 32 B (+16 B on the last step) out.
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_ragged.h"
#include "sage_step_list.h"

namespace sage {

template <int DT>
__global__ void __launch_bounds__(256)
merge_states_kernel(const MergeParams p)
{
    // A row is owned by `cpr_pad` consecutive lanes (cpr rounded up to a power of two <= 64), so all threads of a row
    // sit in ONE wave: every lane's read of lse_acc[row] is issued before the c8 == 0 lane's write of the merged value
    // (wave-lockstep program order).  Spreading a row over waves / workgroups (the round-1 mapping for D = 96, 80, ...)
    // let a later wave read the already-merged lse.
    const int cpr = p.D / 8;                        // 8-channel chunks per row
    const int cpr_pad = p.cpr_pad;
    const long row = (long)blockIdx.x * (256 / cpr_pad) + threadIdx.x / cpr_pad;
    const int c = threadIdx.x % cpr_pad;
    if (row >= (long)p.B * p.H * p.L || c >= cpr) return;
    const int c8 = c * 8;
    const int l = (int)(row % p.L);
    const long bh = row / p.L;
    const int h = (int)(bh % p.H), b = (int)(bh / p.H);

    const uint16_t *on = reinterpret_cast<const uint16_t *>(p.o_new) + (long)b * p.n_sb + (long)h * p.n_sh + (long)l * p.n_sl + c8;
    float *acc = p.o_acc + row * p.D + c8;
    const v4u raw = *reinterpret_cast<const v4u *>(on);
    float xn[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const unsigned w = raw[j >> 1];
        xn[j] = ld16<DT>((uint16_t)((j & 1) ? (w >> 16) : (w & 0xffffu)));
    }
    const float ln = p.lse_new[row];
    float r[8], lse;
    if (p.first) {
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = xn[j];
        lse = ln;
    } else {
        const float la = p.lse_acc[row];
        const float m = fmaxf(la, ln);
        if (m == -INFINITY) {                       // neither side attended to anything: keep the (zero) state
#pragma unroll
            for (int j = 0; j < 8; j++) r[j] = 0.0f;
            lse = -INFINITY;
        } else {
            const float wa = __expf(la - m), wb = __expf(ln - m);
            const float s = wa + wb, inv = 1.0f / s;
            const v4f a0 = *reinterpret_cast<const v4f *>(acc), a1 = *reinterpret_cast<const v4f *>(acc + 4);
#pragma unroll
            for (int j = 0; j < 8; j++) r[j] = ((j < 4 ? a0[j] : a1[j - 4]) * wa + xn[j] * wb) * inv;
            lse = m + __logf(s);
        }
    }
    v4f o0 = {r[0], r[1], r[2], r[3]}, o1 = {r[4], r[5], r[6], r[7]};
    *reinterpret_cast<v4f *>(acc) = o0;
    *reinterpret_cast<v4f *>(acc + 4) = o1;
    if (c8 == 0) p.lse_acc[row] = lse;
    if (p.o_out != nullptr) {
        uint16_t *oo = reinterpret_cast<uint16_t *>(p.o_out) + (long)b * p.o_sb + (long)h * p.o_sh + (long)l * p.o_sl + c8;
        v4u pk;
#pragma unroll
        for (int w = 0; w < 4; w++) pk[w] = (unsigned)st16<DT>(r[2 * w]) | ((unsigned)st16<DT>(r[2 * w + 1]) << 16);
        *reinterpret_cast<v4u *>(oo) = pk;
    }
}

// ---- split-KV merge: S partial states of one attention call -> final output (one pass) ---------------------------------
// The partial outputs are fp16 (11-bit significand: the merge adds no visible rounding for fp16 / bf16 results) in the
// order the attention kernel wrote them with the KV chunks folded into the kv-head dimension: [B, Hkv, S, group, L, D]
// (query head h = hk * group + g), and their log-sum-exps (log2 domain, as the kernel leaves them) [B, Hkv, S, group, L];
// an optional (S+1)-th chunk (a ragged tail of the key range computed by a second launch) comes as [B, H, L, D] / [B, H, L].
// One thread owns 8 channels of one row.  PT: the element type of the partial outputs -- uint16_t (fp16, sage_merge_split) or float (the exact
// split's FP32 partials, sage_merge_split_f32; same arithmetic)
template <typename PT>
__device__ __forceinline__ void ld_part8(const PT *src, float (&x)[8])
{
    if constexpr (sizeof(PT) == 4) {
        const v4f a = *reinterpret_cast<const v4f *>(src), b = *reinterpret_cast<const v4f *>(src + 4);
#pragma unroll
        for (int j = 0; j < 4; j++) { x[j] = a[j]; x[4 + j] = b[j]; }
    } else {
        const v4u raw = *reinterpret_cast<const v4u *>(src);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const unsigned wd = raw[j >> 1];
            x[j] = f16_to_f32((uint16_t)((j & 1) ? (wd >> 16) : (wd & 0xffffu)));
        }
    }
}

// One row of the merge, 8 channels of it: the S partials la[s * HL] / oa[s * HL * D ..] (HL: the chunk stride in rows), an optional tail (ot
// non-null) with LSE lt (-inf without one); the merged channels go to oo, the row's LSE to *lo if lo is non-null.  The arithmetic both merge
// kernels run: the maximum over the LSEs, exp2 of the differences, a chunk of LSE -inf skipped, the sum in the order s = 0 .. S - 1 (tail last),
// one reciprocal, m + log2(wsum).
template <int DT, typename PT>
__device__ __forceinline__ void merge_split_row(const float *la, const PT *oa, long HL, int S, int D, const PT *ot, float lt, uint16_t *oo, float *lo)
{
    const bool tail = ot != nullptr;
    float m = lt;
    for (int s = 0; s < S; s++) m = fmaxf(m, la[(long)s * HL]);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, wsum = 0.0f;
    auto add = [&](const PT *src, float lse) {
        if (lse == -INFINITY) return;                       // chunk with no visible key for this row
        const float w = __builtin_amdgcn_exp2f(lse - m);
        float x[8];
        ld_part8(src, x);
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] += w * x[j];
        wsum += w;
    };
    if (m != -INFINITY) {
        for (int s = 0; s < S; s++) add(oa + (long)s * HL * D, la[(long)s * HL]);
        if (tail) add(ot, lt);
    }
    const float inv = wsum > 0.0f ? 1.0f / wsum : 0.0f;
    v4u pk;
#pragma unroll
    for (int w = 0; w < 4; w++) pk[w] = (unsigned)st16<DT>(acc[2 * w] * inv) | ((unsigned)st16<DT>(acc[2 * w + 1] * inv) << 16);
    *reinterpret_cast<v4u *>(oo) = pk;
    if (lo != nullptr) *lo = wsum > 0.0f ? m + __builtin_amdgcn_logf(wsum) : -INFINITY;   // v_log_f32 = log2
}

template <int DT, typename PT>
__global__ void __launch_bounds__(256)
merge_split_kernel(const SplitMergeParams p)
{
    const int cpr = p.D / 8;
    const int cpr_pad = p.cpr_pad;
    const long row = (long)blockIdx.x * (256 / cpr_pad) + threadIdx.x / cpr_pad;
    const int c = threadIdx.x % cpr_pad;
    if (row >= (long)p.B * p.H * p.L || c >= cpr) return;
    const int c8 = c * 8;
    const int l = (int)(row % p.L);
    const long bh = row / p.L;
    const int h = (int)(bh % p.H), b = (int)(bh / p.H);
    const int hk = h / p.group, gq = h - hk * p.group;
    const long HL = (long)p.group * p.L;                                              // chunk stride in rows
    const long r0 = (((long)b * (p.H / p.group) + hk) * p.S) * HL + (long)gq * p.L + l;   // row of chunk 0
    const float *la = p.lse_part + r0;                                                // + s * HL
    const PT *oa = reinterpret_cast<const PT *>(p.o_part) + r0 * p.D + c8;
    const bool tail = p.o_tail != nullptr;
    const float lt = tail ? p.lse_tail[row] : -INFINITY;
    uint16_t *oo = reinterpret_cast<uint16_t *>(p.o_out) + (long)b * p.o_sb + (long)h * p.o_sh + (long)l * p.o_sl + c8;
    merge_split_row<DT, PT>(la, oa, HL, p.S, p.D, tail ? reinterpret_cast<const PT *>(p.o_tail) + row * p.D + c8 : nullptr, lt, oo,
                            (p.lse_out != nullptr && c8 == 0) ? p.lse_out + row : nullptr);
}

// ---- the split step call's merge: the same rows, for the DECODE sequences of a step alone -------------------------------------
// The partials are the dense workspace of the call -- lse_part [B, Hkv, S, group, L], o_part [.., D] (FP32) with L = min(max_seqlen_q, 32) rows
// per (sequence, head) -- and the results are packed: row l of sequence b lies at packed row first_b + l of o [total_q, H, D] (o_sl / o_sh) and of
// lse [H, total_q] (lse_sh).  One thread owns 8 channels of workspace row (b, h, l); ragged_band with the band (0, 32] decides: a sequence
// outside the band and a row at or beyond n_b are not touched.
template <int DT>
__global__ void __launch_bounds__(256)
merge_split_ragged_kernel(const SplitMergeParams p, const RaggedArgs ra, const int max_seqlen_q, const long lse_sh)
{
    const int cpr = p.D / 8;
    const int cpr_pad = p.cpr_pad;
    const long row = (long)blockIdx.x * (256 / cpr_pad) + threadIdx.x / cpr_pad;
    const int c = threadIdx.x % cpr_pad;
    if (row >= (long)p.B * p.H * p.L || c >= cpr) return;
    const int c8 = c * 8;
    const int l = (int)(row % p.L);
    const long bh = row / p.L;
    const int h = (int)(bh % p.H), b = (int)(bh / p.H);
    int first, nb;
    ragged_band(ra.cu_q[b], ra.cu_q[b + 1], ra.total_q, max_seqlen_q, 0, kStepDecodeRows, first, nb);
    if (l >= nb) return;
    const int hk = h / p.group, gq = h - hk * p.group;
    const long HL = (long)p.group * p.L;                                              // chunk stride in rows
    const long r0 = step_split_ws_row(b, hk, 0, gq, l, p.H / p.group, p.S, p.group, p.L);    // row of chunk 0
    uint16_t *oo = reinterpret_cast<uint16_t *>(p.o_out) + (long)(first + l) * p.o_sl + (long)h * p.o_sh + c8;
    merge_split_row<DT, float>(p.lse_part + r0, reinterpret_cast<const float *>(p.o_part) + r0 * p.D + c8, HL, p.S, p.D, nullptr, -INFINITY, oo,
                               (p.lse_out != nullptr && c8 == 0) ? p.lse_out + (long)h * lse_sh + first + l : nullptr);
}

template <typename PT>
static hipError_t merge_split(const SplitMergeParams &p, hipStream_t stream)
{
    const long rows = (long)p.B * p.H * p.L;
    if (rows <= 0) return hipSuccess;
    SplitMergeParams q = p;
    q.cpr_pad = 1;
    while (q.cpr_pad < p.D / 8) q.cpr_pad *= 2;
    if (q.cpr_pad > 64) return hipErrorInvalidValue;
    const long rpb = 256 / q.cpr_pad;
    const dim3 grid((unsigned)((rows + rpb - 1) / rpb));
    if (p.dtype == DT_F16) hipLaunchKernelGGL((merge_split_kernel<DT_F16, PT>), grid, dim3(256), 0, stream, q);
    else hipLaunchKernelGGL((merge_split_kernel<DT_BF16, PT>), grid, dim3(256), 0, stream, q);
    return hipGetLastError();
}

hipError_t launch_merge_split(const SplitMergeParams &p, hipStream_t stream) { return merge_split<uint16_t>(p, stream); }
hipError_t launch_merge_split_f32(const SplitMergeParams &p, hipStream_t stream) { return merge_split<float>(p, stream); }

// p: o_part / lse_part the workspace (L = its rows per (sequence, head)), o_out / lse_out the packed results (o_sl / o_sh; o_sb unused)
hipError_t launch_merge_split_ragged(const SplitMergeParams &p, const RaggedArgs &r, int max_seqlen_q, long lse_sh, hipStream_t stream)
{
    const long rows = (long)p.B * p.H * p.L;
    if (rows <= 0) return hipSuccess;
    if (r.cu_q == nullptr || r.total_q < 1 || p.L != step_split_ws_rows(max_seqlen_q) || p.o_tail != nullptr) return hipErrorInvalidValue;
    SplitMergeParams q = p;
    q.cpr_pad = 1;
    while (q.cpr_pad < p.D / 8) q.cpr_pad *= 2;
    if (q.cpr_pad > 64) return hipErrorInvalidValue;
    const long rpb = 256 / q.cpr_pad;
    const dim3 grid((unsigned)((rows + rpb - 1) / rpb));
    if (p.dtype == DT_F16) hipLaunchKernelGGL(merge_split_ragged_kernel<DT_F16>, grid, dim3(256), 0, stream, q, r, max_seqlen_q, lse_sh);
    else hipLaunchKernelGGL(merge_split_ragged_kernel<DT_BF16>, grid, dim3(256), 0, stream, q, r, max_seqlen_q, lse_sh);
    return hipGetLastError();
}

hipError_t launch_merge_states(const MergeParams &p, hipStream_t stream)
{
    const long rows = (long)p.B * p.H * p.L;
    if (rows <= 0) return hipSuccess;
    MergeParams q = p;
    q.cpr_pad = 1;
    while (q.cpr_pad < p.D / 8) q.cpr_pad *= 2;
    if (q.cpr_pad > 64) return hipErrorInvalidValue;          // head_dim <= 512 (checked by the C ABI)
    const long rpb = 256 / q.cpr_pad;
    const dim3 grid((unsigned)((rows + rpb - 1) / rpb));
    if (p.dtype == DT_F16) hipLaunchKernelGGL(merge_states_kernel<DT_F16>, grid, dim3(256), 0, stream, q);
    else hipLaunchKernelGGL(merge_states_kernel<DT_BF16>, grid, dim3(256), 0, stream, q);
    return hipGetLastError();
}

}  // namespace sage
