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

// The item's work -- prologue, tile loop, epilogue -- is qk192_item of sage_qk192.h, shared with the packed kernel; this kernel says which item.
template <bool CAUSAL, int DT>
__global__ void __launch_bounds__(256, 2) qk192_attn_kernel(const Qk192AttnParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // ---- work item: query head fastest (a GQA group streams one kv head's images together), the heaviest causal blocks first ----
    const int bid = blockIdx.x;
    const int h = bid % p.Hq, rest = bid / p.Hq;
    const int b = rest % p.B, qr = rest / p.B;
    const int hk = h / p.group;
    Qk192Item it;
    it.qblk = CAUSAL ? p.nqblk - 1 - qr : qr;
    it.Lq = p.Lq; it.Lk = p.Lk; it.shift = 0;
    it.q = reinterpret_cast<const uint16_t *>(p.q) + (long)b * p.q_sb + (long)h * p.q_sh;
    it.q_sl = p.q_sl;
    it.o = reinterpret_cast<unsigned char *>(p.o) + 2 * ((long)b * p.o_sb + (long)h * p.o_sh);
    it.o_sl = p.o_sl;
    it.lse = p.lse != nullptr ? p.lse + ((long)b * p.Hq + h) * (long)p.Lq : nullptr;
    it.k_img = p.k_img + ((long)b * p.Hkv + hk) * p.ntile * QK192_K_TILE_BYTES;
    it.v_img = p.v_img + ((long)b * p.Hkv + hk) * p.ntile * QK192_V_TILE_BYTES;
    it.k_scale = p.k_scale + ((long)b * p.Hkv + hk) * p.ntile * 4;
    it.v_scale = p.v_scale + ((long)b * p.Hkv + hk) * QK192_DV;
    it.sm_scale_log2 = p.sm_scale_log2;
    qk192_item<CAUSAL ? QK192_MASK_TOP_LEFT : QK192_MASK_NONE, DT>(it, smem);
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
