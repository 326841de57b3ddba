// sage_kv_list_plan.hip -- the two work lists of the listed step call on the paged KV cache (include/sage_kvlist_gfx950.h), built on
// the device in ONE small launch so that the call never reads on the host: the decode sequences heaviest first, and every (sequence, 128-row
// query block) of the chunk sequences heaviest first, with the chunk launch's plan {group, fold, left} in the header.  The arithmetic -- classes,
// clamps, weights, ranks, the header -- is csrc/sage_step_list.h's (the host runs the same functions: sage_kvlist_plan_host); this file holds the
// parallel walk alone.  One workgroup: B <= kVarlenPlanMaxSeq; a Hillis-Steele scan in LDS, ranks by the closed-form counts.
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_step_list.h"

namespace sage {

static_assert(kStepHdrWords == kStepListHdrWords, "one header size");

__global__ void __launch_bounds__(1024) kv_list_plan_kernel(const KvListPlanParams p)
{
    __shared__ int sq[2][kVarlenPlanMaxSeq];
    __shared__ int rows_s[kVarlenPlanMaxSeq], lk_s[kVarlenPlanMaxSeq], dw_s[kVarlenPlanMaxSeq];
    __shared__ int max_len, n_decode;
    const int i = threadIdx.x, B = p.B;
    const int cap = step_weight_cap(p.window);
    if (i == 0) { max_len = 0; n_decode = 0; }
    __syncthreads();
    if (i < B) {
        const StepSeq s = step_seq(p.cu_q[i], p.cu_q[i + 1], p.total_q, p.max_seqlen_q, p.kv_lens[i], p.q_start[i], p.Lk, p.window);
        rows_s[i] = s.cls == STEP_CHUNK ? s.rows : 0;
        lk_s[i] = s.lk_eff;
        dw_s[i] = s.cls == STEP_DECODE ? step_decode_weight(s.lk_eff, cap) : -1;
        sq[0][i] = step_blocks(rows_s[i]);
        if (s.cls == STEP_CHUNK) atomicMax(&max_len, s.len);
        if (s.cls == STEP_DECODE) atomicAdd(&n_decode, 1);
    }
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < B; d <<= 1) {                    // inclusive scan of the chunk sequences' block counts
        if (i < B) sq[cur ^ 1][i] = sq[cur][i] + (i >= d ? sq[cur][i - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    // (the grid's size check of the entry bounds B * ceil(max_seqlen_q / 128), and with it this sum, below 2^31)
    const int nitems_all = sq[cur][B - 1];
    const int nitems = min(max(nitems_all, 0), max(p.items_cap, 0));
    int *const decode_list = p.ws + kStepHdrWords, *const items = decode_list + B;
    if (i == 0) step_write_hdr(p.ws, n_decode, nitems_all, p.items_cap, max_len, p.Hq, p.Hkv, p.head_dim);
    // a total order over the decode sequences: every rank in [0, n_decode) is taken once, and n_decode <= B
    if (i < B && dw_s[i] >= 0) decode_list[step_decode_rank(dw_s, B, i)] = i;
    // the first t with scan[t] > idx owns block idx
    for (int idx = i; idx < nitems_all; idx += 1024) {
        int lo = 0, hi = B - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sq[cur][mid] > idx) hi = mid; else lo = mid + 1;
        }
        const int j = idx - (lo > 0 ? sq[cur][lo - 1] : 0);
        const int rank = step_chunk_rank(rows_s, lk_s, B, lo, j, cap);
        // the words come from the device, the workspace was sized on the host: a malformed prefix array (overlapping sequences) is clamped to the
        // cap -- work is dropped (the call's result is then as undefined as its input), nothing is written out of bounds
        if (rank >= 0 && rank < nitems) {
            items[2 * rank] = lo;
            items[2 * rank + 1] = j;
        }
    }
}

hipError_t launch_kv_list_plan(const KvListPlanParams &p, hipStream_t stream)
{
    if (p.B <= 0 || p.B > kVarlenPlanMaxSeq || p.ws == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kv_list_plan_kernel, dim3(1), dim3(1024), 0, stream, p);
    return hipGetLastError();
}

}  // namespace sage
