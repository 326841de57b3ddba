// sage_qk192_varlen_attn.hip -- the PACKED (variable-length) attention launch of the 192-wide Q / K, 128-wide V route on gfx950
// (include/sage_qk192v_gfx950.h).  The work of an item -- 128 query rows of one query head, the MFMA products, the two two-slot
// rings and their counted waits -- is qk192_item of sage_qk192.h, the dense kernel's; this kernel finds the item.
//
//  * workgroup bid: query head bid % Hq (a GQA group's heads adjacent: they stream one kv head's tiles together), item bid / Hq of the device's
//    work list, heaviest first.  The grid is sized on the host for ceil(total_q / 128) + nseq items; workgroups beyond hdr[0] exit.
//  * geometry from the prefix arrays: Lq_s, Lk_s, the row base cu_q[s], the tile base cu_kt[s], shift = Lk_s - Lq_s under the bottom-right
//    mask.  All of it is made wave-uniform (readfirstlane), so the K-scale loads of the loop, 4 (cu_kt[s] + t), stay scalar loads: a vector
//    load there would join the tile DMA's in-order counter.
//  * an item with kend <= 0 -- a block wholly in front of key 0, or a sequence without keys -- has no tile in the images.  It leaves BEFORE
//    qk192_item: it writes +0 and lse = -inf for its rows and requests nothing.  The test is workgroup-uniform (it depends on the block, not
//    on the wave), so every item that reaches qk192_item has kend >= 1 and issues the unconditional prologue of tile 0: the counted-wait
//    argument there starts from the same five DMA instructions as the dense kernel's, with nothing of this kernel counted in front of them
//    (the plan and prefix loads are scalar; were they vector loads, they are older than the prologue's requests and their values were
//    consumed to form its addresses, so the in-order counter has retired them).
//  * a negative shift (more rows than keys) leaves the first rows of a block without a key while later rows have some: qk192_item masks
//    their P before the row sum, and their running maximum stays at its start value.
//  * every row, tile and item index derived from cu_seqlens is clamped to total_q / total_k / the capacities before it addresses anything.
#include "../../include/sage_qk192v_gfx950.h"
#include "sage_qk192.h"
#include "sage_host_checks.h"

namespace sage {

template <int MASK, int DT>
__global__ void __launch_bounds__(256, 2) qk192_varlen_attn_kernel(const Qk192vAttnParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int bid = blockIdx.x;
    const int h = bid % p.Hq, idx = bid / p.Hq;
    if (idx >= p.plan[p.lay.hdr()]) return;
    auto uni = [](int x) { return __builtin_amdgcn_readfirstlane(x); };
    const int s = uni(p.plan[p.lay.items() + 2 * idx]), blk = uni(p.plan[p.lay.items() + 2 * idx + 1]);
    const int q0 = min(max(uni(p.cu_q[s]), 0), p.total_q);
    const int lq = min(max(uni(p.cu_q[s + 1] - p.cu_q[s]), 0), p.total_q - q0);
    const int kt0 = uni(p.plan[p.lay.cu_kt() + s]);
    const int k0 = min(max(uni(p.cu_k[s]), 0), p.total_k);
    int lk = min(max(uni(p.cu_k[s + 1] - p.cu_k[s]), 0), p.total_k - k0);
    lk = min(lk, BLKK * max(p.lay.tiles_cap - kt0, 0));                   // (the tiles the images hold behind cu_kt[s])
    const int shift = MASK == QK192_MASK_BOTTOM_RIGHT ? lk - lq : 0;
    const int kend = MASK != QK192_MASK_NONE ? min(lk, blk * BLKQ + BLKQ + shift) : lk;
    const int hk = h / p.group;
    unsigned char *o = reinterpret_cast<unsigned char *>(p.o) + 2 * ((long)q0 * p.o_sl + (long)h * p.o_sh);
    float *lse = p.lse != nullptr ? p.lse + (long)h * p.total_q + q0 : nullptr;
    if (blk < 0 || blk * BLKQ >= lq || kt0 < 0) return;                   // (no row, or a wrapped tile prefix: a plan built from a malformed cu_seqlens)
    if (kend <= 0) {
        // no visible key: sixteen threads write a row of 256 zero bytes, thread r the LSE of row r
        const int tid = threadIdx.x;
        const v4u zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int pass = 0; pass < 8; pass++) {
            const int row = blk * BLKQ + 16 * pass + (tid >> 4);
            if (row < lq) *reinterpret_cast<v4u *>(o + 2 * ((long)row * p.o_sl) + (tid & 15) * 16) = zero;
        }
        if (lse != nullptr && tid < BLKQ && blk * BLKQ + tid < lq) lse[blk * BLKQ + tid] = -INFINITY;
        return;
    }
    Qk192Item it;
    it.qblk = blk; it.Lq = lq; it.Lk = lk; it.shift = shift;
    it.q = reinterpret_cast<const uint16_t *>(p.q) + (long)q0 * p.q_sl + (long)h * p.q_sh;
    it.q_sl = p.q_sl;
    it.o = o;
    it.o_sl = p.o_sl;
    it.lse = lse;
    const long tile0 = (long)hk * p.lay.tiles_cap + kt0;
    it.k_img = p.k_img + tile0 * QK192_K_TILE_BYTES;
    it.v_img = p.v_img + tile0 * QK192_V_TILE_BYTES;
    it.k_scale = p.k_scale + tile0 * 4;
    it.v_scale = p.v_scale + ((long)s * p.Hkv + hk) * QK192_DV;
    it.sm_scale_log2 = p.sm_scale_log2;
    qk192_item<MASK, DT>(it, smem);
}

hipError_t launch_qk192v_attn(const Qk192vAttnParams &p, int mask, int dtype, hipStream_t stream)
{
    const dim3 grid((unsigned)((long)p.lay.items_cap * p.Hq)), block(256);
#define SAGE_QK192V_LAUNCH(M, T) hipLaunchKernelGGL((qk192_varlen_attn_kernel<M, T>), grid, block, QK192_LDS_BYTES, stream, p)
#define SAGE_QK192V_DT(M) do { if (dtype == DT_F16) SAGE_QK192V_LAUNCH(M, DT_F16); else SAGE_QK192V_LAUNCH(M, DT_BF16); } while (0)
    if (mask == QK192_MASK_NONE) SAGE_QK192V_DT(QK192_MASK_NONE);
    else if (mask == QK192_MASK_TOP_LEFT) SAGE_QK192V_DT(QK192_MASK_TOP_LEFT);
    else SAGE_QK192V_DT(QK192_MASK_BOTTOM_RIGHT);
#undef SAGE_QK192V_DT
#undef SAGE_QK192V_LAUNCH
    return hipGetLastError();
}

}  // namespace sage

extern "C" {

using namespace sage;

SAGE_QK192V_API int sage_qk192v_attn(const void *q, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, const void *k_image,
                                     const void *v_image, const float *k_scale, const float *v_scale, const void *ws, int64_t ws_bytes,
                                     void *o, float *lse, int nseq, int total_q, int total_k, int Hq, int Hkv, int head_dim_qk, int head_dim_v,
                                     int64_t q_sl, int64_t q_sh, int64_t o_sl, int64_t o_sh, int mask, float sm_scale, int dtype, void *stream)
{
    const char *const e = "sage_qk192v_attn";
    SAGE_REQUIRE(head_dim_qk == QK192_DQK && head_dim_v == QK192_DV,
                 "%s: head_dim_qk must be 192 and head_dim_v 128 (got %d and %d); zero-pad 129 .. 191 / 1 .. 127, and call sage_attn_fused_qblock_pv_f8_varlen for 64 / 128",
                 e, head_dim_qk, head_dim_v);
    SAGE_REQUIRE(dtype == DT_F16 || dtype == DT_BF16, "%s: dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got %d)", e, dtype);
    SAGE_REQUIRE(mask >= 0 && mask <= 2, "%s: mask must be 0 (none), 1 (causal top-left) or 2 (causal bottom-right) (got %d)", e, mask);
    SAGE_REQUIRE(Hq >= 1 && Hkv >= 1 && total_q >= 1 && total_k >= 1, "%s: empty problem (Hq %d, Hkv %d, total_q %d, total_k %d)", e, Hq, Hkv, total_q, total_k);
    SAGE_REQUIRE(nseq >= 1 && nseq <= 1024, "%s: nseq must be in 1 .. 1024 (got %d)", e, nseq);
    SAGE_REQUIRE(Hq % Hkv == 0, "%s: Hq (%d) must be a multiple of Hkv (%d)", e, Hq, Hkv);
    SAGE_REQUIRE(q && cu_seqlens_q && cu_seqlens_k && k_image && v_image && k_scale && v_scale && ws && o, "%s: null pointer (only lse may be null)", e);
    SAGE_REQUIRE(aligned16_strides(q, 8, q_sl, q_sh) && aligned16_strides(o, 8, o_sl, o_sh) && q_sl >= 0 && o_sl >= 0 && q_sh >= QK192_DQK && o_sh >= QK192_DV,
                 "%s: q and o must be 16-byte aligned with non-negative strides in multiples of 8 elements and a head stride of at least 192 (q) / 128 (o)", e);
    SAGE_REQUIRE(aligned16(k_image) && aligned16(v_image) && aligned16(v_scale) && aligned16(ws) && aligned4(k_scale) && aligned4(lse) &&
                 aligned4(cu_seqlens_q) && aligned4(cu_seqlens_k),
                 "%s: the images, v_scale and ws must be 16-byte aligned, k_scale, lse and cu_seqlens 4-byte", e);
    const int64_t need = sage_qk192v_ws_bytes(nseq, Hkv, total_q, total_k);
    SAGE_REQUIRE(ws_bytes >= need, "%s: ws holds %lld bytes, sage_qk192v_ws_bytes(nseq, Hkv, total_q, total_k) = %lld", e, (long long)ws_bytes, (long long)need);
    Qk192vAttnParams p{};
    p.lay = qk192v_plan(nseq, total_q, total_k);
    SAGE_REQUIRE((int64_t)p.lay.items_cap * Hq < ((int64_t)1 << 31), "%s: Hq * (ceil(total_q / 128) + nseq) must be below 2^31", e);
    p.q = q; p.cu_q = cu_seqlens_q; p.cu_k = cu_seqlens_k; p.plan = static_cast<const int32_t *>(ws);
    p.k_img = static_cast<const unsigned char *>(k_image); p.v_img = static_cast<const unsigned char *>(v_image);
    p.k_scale = k_scale; p.v_scale = v_scale; p.o = o; p.lse = lse;
    p.q_sl = q_sl; p.q_sh = q_sh; p.o_sl = o_sl; p.o_sh = o_sh;
    p.Hq = Hq; p.Hkv = Hkv; p.group = Hq / Hkv; p.total_q = total_q; p.total_k = total_k;
    p.sm_scale_log2 = sm_scale * 1.44269504088896340736f;      // in FP32, as the dense call forms it
    const hipError_t err = launch_qk192v_attn(p, mask, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
