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
//
// The kernel's text is mla_decode_body<DT, false> of sage_mla_loop.h, which it shares with pass 2 of the exact split of the key range
// (sage_mla_split.hip); this unit keeps the launcher, the LDS opt-in and the C entry points.
#include "../../include/sage_mla_gfx950.h"
#include "sage_mla_loop.h"
#include "sage_host_checks.h"
#include "sage_quant_math.h"

#include <atomic>

namespace sage {

template <int DT>
__global__ void __launch_bounds__(256, 1) mla_decode_kernel(const MlaAttnParams p)
{
    mla_decode_body<DT, false>(p);
}

hipError_t launch_mla_attn(const MlaAttnParams &p, int dtype, hipStream_t stream)
{
    const dim3 grid((unsigned)((long)p.B * p.nblk)), block(256);
    if (dtype == DT_F16) hipLaunchKernelGGL(mla_decode_kernel<DT_F16>, grid, block, MLA_LDS_BYTES, stream, p);
    else hipLaunchKernelGGL(mla_decode_kernel<DT_BF16>, grid, block, MLA_LDS_BYTES, stream, p);
    return hipGetLastError();
}

// Dynamic shared memory above the 64 KiB a kernel gets unasked (136 KiB here, 72 KiB for pass 1 of the split): the attribute is set once per
// process and device (lock-free: a race repeats the idempotent calls; `done` has a bit per device ordinal mod 64), and a device that offers less
// than `bytes` is refused.  0 = ready; otherwise the message is set.
int mla_raise_lds(const char *e, std::atomic<unsigned long long> &done, int bytes, const void *const *kernels, const int *kernel_bytes, int count)
{
    int dev = -1, lds = 0, optin = 0;
    hipError_t err = hipGetDevice(&dev);
    if (err != hipSuccess || dev < 0) return set_last_error(SAGE_EINVAL, "%s: no current device: %s", e, hipGetErrorString(err));
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_relaxed) & bit) return 0;
    err = hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    if (err != hipSuccess) return set_last_error(SAGE_EINVAL, "%s: cannot read the device's LDS size: %s", e, hipGetErrorString(err));
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) (void)hipGetLastError();
    if (optin > lds) lds = optin;
    if (lds < bytes)
        return set_last_error(SAGE_EINVAL, "%s: the device offers %d bytes of LDS per workgroup, the kernel needs %d", e, lds, bytes);
    for (int i = 0; i < count && err == hipSuccess; i++)
        err = hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, kernel_bytes[i]);
    if (err != hipSuccess)
        return set_last_error(SAGE_EINVAL, "%s: cannot raise the kernel's dynamic LDS to %d bytes: %s", e, bytes, hipGetErrorString(err));
    done.fetch_or(bit, std::memory_order_relaxed);
    return 0;
}

static int mla_lds_ready(const char *e)
{
    static std::atomic<unsigned long long> done{0};
    static const void *const kernels[2] = {reinterpret_cast<const void *>(&mla_decode_kernel<DT_F16>),
                                           reinterpret_cast<const void *>(&mla_decode_kernel<DT_BF16>)};
    static const int bytes[2] = {MLA_LDS_BYTES, MLA_LDS_BYTES};
    return mla_raise_lds(e, done, MLA_LDS_BYTES, kernels, bytes, 2);
}

// the argument checks of sage_mla_attn up to (not including) the device's LDS, in the header's order, and the parameter block they allow:
// sage_mlasplit_attn (sage_mla_split.hip) refuses the same things in the same words under its own name
int mla_attn_prepare(const char *e, const void *q, const void *k_image, const void *v_image, const float *k_scale, const float *v_scale,
                     const int32_t *kv_lens, void *o, float *lse, int B, int Lq, int Hq, int Lk, int width_qk, int width_v, int64_t q_sb,
                     int64_t q_sl, int64_t q_sh, float sm_scale, int dtype, MlaAttnParams &p)
{
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
    p = MlaAttnParams{};
    p.q = q; p.k_img = static_cast<const unsigned char *>(k_image); p.v_img = static_cast<const unsigned char *>(v_image);
    p.k_scale = k_scale; p.v_scale = v_scale; p.kv_lens = kv_lens; p.o = o; p.lse = lse;
    p.q_sb = q_sb; p.q_sl = q_sl; p.q_sh = q_sh;
    p.B = B; p.Lq = Lq; p.Hq = Hq; p.Lk = Lk; p.rows = (int)rows; p.nblk = (int)nblk; p.ntile = (Lk + BLKK - 1) / BLKK;
    p.sm_scale_log2 = sm_scale * 1.44269504088896340736f;      // in FP32, as the reference's kernel forms it (qk_int_sv_f8_cuda_sm89.cuh:90)
    return SAGE_OK;
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
    MlaAttnParams p;
    if (mla_attn_prepare(e, q, k_image, v_image, k_scale, v_scale, kv_lens, o, lse, B, Lq, Hq, Lk, width_qk, width_v, q_sb, q_sl, q_sh, sm_scale,
                         dtype, p) != SAGE_OK)
        return SAGE_EINVAL;
    if (mla_lds_ready(e) != 0) return SAGE_EINVAL;
    const hipError_t err = launch_mla_attn(p, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
