// sage_qk192_varlen_prepass.hip -- the plan and the K / V pre-pass of the PACKED 192-wide Q / K, 128-wide V route
// (include/sage_qk192v_gfx950.h), gfx950.  Four launches, none of which the host waits for:
//   1. launch_varlen_plan (sage_varlen_plan.hip)  the tile prefix cu_kt, the (sequence, 128-row block) work list and its count
//   2. qk192v_maps_kernel   what that plan has not: the prefix of 256-token statistics chunks (its slabs are the family's 512), the
//                           tile -> sequence and chunk -> sequence maps, the clamped counts, and zeros for the mean and V scale of a
//                           sequence without keys (no chunk and no tile of it exists to write them)
//   3. qk192v_stats_kernel  one workgroup per (chunk of a sequence, kv head): qk192_stats_chunk on the sequence's slice
//   4. qk192v_quant_kernel  one workgroup per (tile of a sequence, kv head): qk192_quant_tile on the sequence's slice
// Chunks and tiles count from the sequence's own first key and fold in ascending order, so the statistics and images of a sequence are bit for
// bit those of the dense pre-pass on its slice.  The grids are sized on the host for tiles_cap / chunks_cap; workgroups beyond the device's
// counts exit.  Every row and every count derived from cu_seqlens is clamped to total_k and the capacities before it addresses anything.
#include "../../include/sage_qk192v_gfx950.h"
#include "sage_qk192.h"
#include "sage_qk192_prep.h"
#include "sage_host_checks.h"
#include "sage_kernels.h"

namespace sage {

__global__ void __launch_bounds__(1024) qk192v_maps_kernel(const Qk192vPrepParams p)
{
    __shared__ int sc[2][kVarlenPlanMaxSeq], skt[kVarlenPlanMaxSeq];
    const int i = threadIdx.x, nseq = p.lay.nseq;
    int32_t *plan = p.plan;
    int lk = 0;
    if (i < nseq) {
        lk = p.cu_k[i + 1] - p.cu_k[i];
        lk = lk > 0 ? lk : 0;                                // (as launch_varlen_plan counts its tiles)
        sc[0][i] = (lk + QK192_CHUNK - 1) / QK192_CHUNK;
        skt[i] = plan[p.lay.cu_kt() + i + 1];                // inclusive tile scan
    }
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < nseq; d <<= 1) {
        if (i < nseq) sc[cur ^ 1][i] = sc[cur][i] + (i >= d ? sc[cur][i - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    const int ntiles = min(skt[nseq - 1], p.lay.tiles_cap), nchunks = min(sc[cur][nseq - 1], p.lay.chunks_cap);
    if (i < nseq) plan[p.lay.cu_ch() + i + 1] = sc[cur][i];
    if (i == 0) {
        plan[p.lay.cu_ch()] = 0;
        plan[p.lay.cnt()] = ntiles;
        plan[p.lay.cnt() + 1] = nchunks;
    }
    // the first sequence whose inclusive scan value exceeds idx owns tile / chunk idx
    auto owner = [&](const int *scan, int idx) {
        int lo = 0, hi = nseq - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (scan[mid] > idx) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    for (int idx = i; idx < ntiles; idx += 1024) plan[p.lay.kt_seq() + idx] = owner(skt, idx);
    for (int idx = i; idx < nchunks; idx += 1024) plan[p.lay.ch_seq() + idx] = owner(sc[cur], idx);
    if (i < nseq && lk == 0) {
        for (int e = 0; e < p.Hkv * QK192_DQK; e++) reinterpret_cast<uint16_t *>(p.k_mean)[(long)i * p.Hkv * QK192_DQK + e] = 0;
        for (int e = 0; e < p.Hkv * QK192_DV; e++) p.v_scale[(long)i * p.Hkv * QK192_DV + e] = 0.0f;
    }
}

// the slice of sequence s: its first row and its length, inside the total_k rows whatever cu_seqlens_k says
__device__ __forceinline__ void qk192v_key_slice(const Qk192vPrepParams &p, int s, int &k0, int &lk)
{
    k0 = min(max(p.cu_k[s], 0), p.total_k);
    lk = min(max(p.cu_k[s + 1] - p.cu_k[s], 0), p.total_k - k0);
}

template <int DT>
__global__ void __launch_bounds__(256) qk192v_stats_kernel(const Qk192vPrepParams p)
{
    const int c = blockIdx.x, hk = blockIdx.y;
    if (c >= p.plan[p.lay.cnt() + 1]) return;
    const int s = p.plan[p.lay.ch_seq() + c];
    int k0, lk;
    qk192v_key_slice(p, s, k0, lk);
    if (c < p.plan[p.lay.cu_ch() + s]) return;               // (a prefix that wrapped: a malformed cu_seqlens_k)
    qk192_stats_chunk<DT>(reinterpret_cast<const uint16_t *>(p.k) + (long)k0 * p.k_sl + (long)hk * p.k_sh,
                          reinterpret_cast<const uint16_t *>(p.v) + (long)k0 * p.v_sl + (long)hk * p.v_sh, p.k_sl, p.v_sl,
                          c - p.plan[p.lay.cu_ch() + s], lk, p.ws + ((long)hk * p.lay.chunks_cap + c) * QK192_WS_PER_CHUNK);
}

template <int DT>
__global__ void __launch_bounds__(256) qk192v_quant_kernel(const Qk192vPrepParams p)
{
    const int t = blockIdx.x, hk = blockIdx.y;
    if (t >= p.plan[p.lay.cnt()]) return;
    const int s = p.plan[p.lay.kt_seq() + t];
    int k0, lk;
    qk192v_key_slice(p, s, k0, lk);
    const int c0 = p.plan[p.lay.cu_ch() + s];
    if (t < p.plan[p.lay.cu_kt() + s] || c0 < 0) return;     // (a prefix that wrapped: a malformed cu_seqlens_k)
    const int nchunk = max(min(p.plan[p.lay.cu_ch() + s + 1], p.plan[p.lay.cnt() + 1]) - c0, 0);
    Qk192TileOut out;
    out.k_mean = reinterpret_cast<uint16_t *>(p.k_mean) + ((long)s * p.Hkv + hk) * QK192_DQK;
    out.v_scale = p.v_scale + ((long)s * p.Hkv + hk) * QK192_DV;
    out.k_scale = p.k_scale + ((long)hk * p.lay.tiles_cap + t) * 4;
    out.k_img = p.k_img + ((long)hk * p.lay.tiles_cap + t) * QK192_K_TILE_BYTES;
    out.v_img = p.v_img + ((long)hk * p.lay.tiles_cap + t) * QK192_V_TILE_BYTES;
    qk192_quant_tile<DT>(reinterpret_cast<const uint16_t *>(p.k) + (long)k0 * p.k_sl + (long)hk * p.k_sh,
                         reinterpret_cast<const uint16_t *>(p.v) + (long)k0 * p.v_sl + (long)hk * p.v_sh, p.k_sl, p.v_sl,
                         t - p.plan[p.lay.cu_kt() + s], lk, p.ws + ((long)hk * p.lay.chunks_cap + c0) * QK192_WS_PER_CHUNK, nchunk,
                         p.smooth_k != 0, out);
}

hipError_t launch_qk192v_prepass(const Qk192vPrepParams &p, int dtype, hipStream_t stream)
{
    VarlenPlanParams vp{};
    vp.cu_q = p.cu_q; vp.cu_k = p.cu_k; vp.nseq = p.lay.nseq; vp.blkq = BLKQ; vp.blkk = BLKK; vp.total_k = p.total_k;
    vp.causal = p.mask; vp.Hq = p.Hq; vp.Hkv = p.Hkv; vp.head_dim = 128; vp.pv_fp8 = 1;       // (head_dim: the plan's group / fold only, which this route does not read)
    vp.cu_ks = p.plan + p.lay.cu_kt(); vp.items = p.plan + p.lay.items(); vp.hdr = p.plan + p.lay.hdr();
    vp.items_cap = p.lay.items_cap; vp.forced_group = -1;
    const hipError_t err = launch_varlen_plan(vp, stream);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(qk192v_maps_kernel, dim3(1), dim3(1024), 0, stream, p);
    const dim3 g1(p.lay.chunks_cap, p.Hkv), g2(p.lay.tiles_cap, p.Hkv);
    if (dtype == DT_F16) {
        hipLaunchKernelGGL(qk192v_stats_kernel<DT_F16>, g1, dim3(256), 0, stream, p);
        hipLaunchKernelGGL(qk192v_quant_kernel<DT_F16>, g2, dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(qk192v_stats_kernel<DT_BF16>, g1, dim3(256), 0, stream, p);
        hipLaunchKernelGGL(qk192v_quant_kernel<DT_BF16>, g2, dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace sage

extern "C" {

using namespace sage;

SAGE_QK192V_API int sage_qk192v_abi_version(void) { return SAGE_QK192V_ABI_VERSION; }

SAGE_QK192V_API int64_t sage_qk192v_ws_bytes(int nseq, int Hkv, int total_q, int total_k)
{
    if (nseq < 1 || nseq > kVarlenPlanMaxSeq || Hkv < 1 || total_q < 1 || total_k < 1)
        return set_last_error(SAGE_EINVAL, "sage_qk192v_ws_bytes: empty problem or nseq above %d (nseq %d, Hkv %d, total_q %d, total_k %d)",
                              kVarlenPlanMaxSeq, nseq, Hkv, total_q, total_k);
    const Qk192vPlan lay = qk192v_plan(nseq, total_q, total_k);
    return 4 * (lay.ints() + (int64_t)Hkv * lay.chunks_cap * QK192_WS_PER_CHUNK);
}

SAGE_QK192V_API int sage_qk192v_prepass(const void *k, const void *v, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k,
                                        void *k_image, float *k_scale, void *k_mean, void *v_image, float *v_scale, void *ws, int64_t ws_bytes,
                                        int nseq, int total_q, int total_k, int Hq, int Hkv, int head_dim_qk, int head_dim_v,
                                        int64_t k_sl, int64_t k_sh, int64_t v_sl, int64_t v_sh, int mask, int smooth_k, int dtype, void *stream)
{
    const char *const e = "sage_qk192v_prepass";
    SAGE_REQUIRE(head_dim_qk == QK192_DQK && head_dim_v == QK192_DV,
                 "%s: head_dim_qk must be 192 and head_dim_v 128 (got %d and %d); zero-pad 129 .. 191 / 1 .. 127, and call sage_prepass_kv_varlen's family for 64 / 128",
                 e, head_dim_qk, head_dim_v);
    SAGE_REQUIRE(dtype == DT_F16 || dtype == DT_BF16, "%s: dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got %d)", e, dtype);
    SAGE_REQUIRE(mask >= 0 && mask <= 2, "%s: mask must be 0 (none), 1 (causal top-left) or 2 (causal bottom-right) (got %d)", e, mask);
    SAGE_REQUIRE(Hq >= 1 && Hkv >= 1 && total_q >= 1 && total_k >= 1, "%s: empty problem (Hq %d, Hkv %d, total_q %d, total_k %d)", e, Hq, Hkv, total_q, total_k);
    SAGE_REQUIRE(nseq >= 1 && nseq <= kVarlenPlanMaxSeq, "%s: nseq must be in 1 .. %d (got %d)", e, kVarlenPlanMaxSeq, nseq);
    SAGE_REQUIRE(Hq % Hkv == 0, "%s: Hq (%d) must be a multiple of Hkv (%d)", e, Hq, Hkv);
    SAGE_REQUIRE(k && v && cu_seqlens_q && cu_seqlens_k && k_image && k_scale && k_mean && v_image && v_scale && ws, "%s: null pointer", e);
    SAGE_REQUIRE(aligned16_strides(k, 8, k_sl, k_sh) && aligned16_strides(v, 8, v_sl, v_sh) && k_sl >= 0 && v_sl >= 0 && k_sh >= QK192_DQK && v_sh >= QK192_DV,
                 "%s: k and v must be 16-byte aligned with non-negative strides in multiples of 8 elements and a head stride of at least 192 (k) / 128 (v)", e);
    SAGE_REQUIRE(aligned16(k_image) && aligned16(v_image) && aligned16(ws) && aligned4(k_scale) && aligned4(v_scale) && aligned4(cu_seqlens_q) &&
                 aligned4(cu_seqlens_k) && (reinterpret_cast<uintptr_t>(k_mean) & 1u) == 0,
                 "%s: the images and ws must be 16-byte aligned, k_scale, v_scale and cu_seqlens 4-byte, k_mean 2-byte", e);
    const int64_t need = sage_qk192v_ws_bytes(nseq, Hkv, total_q, total_k);
    SAGE_REQUIRE(ws_bytes >= need, "%s: ws holds %lld bytes, sage_qk192v_ws_bytes(nseq, Hkv, total_q, total_k) = %lld", e, (long long)ws_bytes, (long long)need);
    SAGE_REQUIRE(Hkv <= 65535, "%s: Hkv must be at most 65535 (got %d)", e, Hkv);
    Qk192vPrepParams p{};
    p.lay = qk192v_plan(nseq, total_q, total_k);
    p.k = k; p.v = v; p.cu_q = cu_seqlens_q; p.cu_k = cu_seqlens_k;
    p.plan = static_cast<int32_t *>(ws); p.ws = static_cast<float *>(ws) + p.lay.ints();
    p.k_img = static_cast<unsigned char *>(k_image); p.v_img = static_cast<unsigned char *>(v_image);
    p.k_scale = k_scale; p.v_scale = v_scale; p.k_mean = k_mean;
    p.k_sl = k_sl; p.k_sh = k_sh; p.v_sl = v_sl; p.v_sh = v_sh;
    p.Hq = Hq; p.Hkv = Hkv; p.total_q = total_q; p.total_k = total_k; p.mask = mask; p.smooth_k = smooth_k != 0;
    const hipError_t err = launch_qk192v_prepass(p, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
