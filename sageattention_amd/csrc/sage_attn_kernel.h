// sage_attn_kernel.h -- fused INT8-QK^T / online-softmax / FP8-or-FP16-PV attention for gfx950: the kernel family and its launcher.
// Included by the instantiation units sage_attn_d{128,64}_{f8,f8f,f16}.hip (one per head size, PV format and FP8 score form, so that they
// compile in parallel); sage_attn.hip holds the host-side dispatch.  The kernel's BODY is the fragment sage_attn_body.h, included by the four
// entries at the end of this file: sage_attn_kernel<FORM>, its paged twin sage_attn_paged_kernel<FORM>, that one's ragged
// twin sage_attn_paged_varlen_kernel<FORM> and the ragged twin behind a band filter, sage_attn_paged_step_kernel<FORM> (3.22).
//
// Replaces (behaviourally, not textually) the reference kernels
//   csrc/qattn/qk_int_sv_f8_cuda_sm89.cuh:46-704   (INT8 QK, FP8 PV, two-level accumulation)
//   csrc/qattn/qk_int_sv_f8_cuda_sm90.cu:127-567   (same, 128-key tiles, RO += RO_temp per tile)
//   csrc/qattn/qk_int_sv_f16_cuda_sm80.cu:46-671   (INT8 QK, FP16 PV)
//   sageattention/triton/attn_qk_int8_per_block*.py, attn_qk_int8_block_varlen.py (+causal)
// with one CDNA4 kernel family.  Design:
//
//  * workgroup = 4 waves = 128 query rows of one (batch, q-head); wave w owns rows 32w..32w+31.
//  * swapped product S^T = K Q^T on v_mfma_i32_32x32x32_i8: A = K tile rows from LDS, B = Q
//    fragments kept in VGPRs for the whole kernel.  In the 32x32 C layout a lane then holds 16
//    keys of ONE query row (col = lane&31), so row max / row sum are in-lane chains plus one
//    v_permlane32_swap with the lane^32 partner.
//  * P is converted in registers (v_cvt_pk_fp8_f32 / cvt f16) and is already the B operand of
//    O^T = V^T P^T: the V pre-pass stores V^T tiles in the matching "position" order
//    (sage_common.h), so P never goes through LDS.  FP8 PV runs on the K = 64 instruction
//    v_mfma_f32_32x32x64_f8f6f4 (the plain form: no block scales), twice the rate of the 32x32x16 fp8 MFMA.
//  * one loop iteration covers one 64-key image; scales and masks are per 64-key block.  Two-level
//    accumulation: whole unmasked tiles add their P.V product to the FP32 running output through the
//    MFMA's FP32 C operand (O = O*alpha + sum p v); general tiles start from a zero accumulator and fold
//    it in with one FMA per element (O = O*alpha + T).
//  * K/V tiles live in a 3-slot LDS ring and arrive by LDS-DMA (global_load_lds_dwordx4) two tiles ahead; the
//    K image is XOR-swizzled through the per-lane SOURCE address, the V image is pre-swizzled
//    by the pre-pass: every MFMA operand read is a conflict-free ds_read_b128.
//  * whole unmasked tiles run software-pipelined loops whose instruction order is pinned in asm (six bodies
//    per trip: ring slot and score-register set are compile-time constants in each) -- the fragments
//    sage_attn_loop_f8.h / sage_attn_loop_f16.h, included inside the kernel body.  A work item's last tiles
//    -- the two diagonal tiles of a causal block, the last whole tiles and the ragged tile of a non-causal call --
//    run the same body in three more KINDs behind the loop (nothing more requested, scores behind the diagonal or
//    past Lk masked in front of the row maximum; DIAG_PIPE / TAIL_PIPE below say for which instantiations); what
//    is left -- attn_mask variants, causal blocks ending in a partial tile, ragged FP16-PV tails, D = 64 FP16 PV,
//    sequences under two tiles -- runs the general, phased iteration (tile_iter).
//  * output tile is transposed through (now free) LDS and stored as whole rows, 16 B per lane.
#pragma once
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_attn_form.h"
#include "sage_attn_parts.h"
#include "sage_quant_math.h"
#include "sage_work_order.h"
#include "sage_ragged.h"
#include "sage_step_list.h"
#include <atomic>
#include <climits>
#include <cstdlib>
#include <type_traits>

// ---- build-time switches --------------------------------------------------------------------------
// Rounds 1-5 carried an A/B ladder of ~20 switches here (SAGE_GLDS, SAGE_MXPV, SAGE_KPRELOAD, SAGE_STEADY, SAGE_STAGES, SAGE_NH_F8, SAGE_MAGIC,
// SAGE_PIPE, SAGE_PIPE16, SAGE_PLAIN_PV, SAGE_GRP4, SAGE_RSUM_MFMA, SAGE_FOLDBIAS, SAGE_DIRECT, SAGE_PERS_QF, SAGE_PERS_CAUSAL); every one is
// folded to the value that shipped and its alternative body deleted (round 6).  The last tree that still builds them:
// `git show b0d43f7:sageattention_amd/csrc/sage_attn_kernel.h`; what each measured is in DESIGN.md 3.1 / 3.7 / 3.8.  What is fixed now: K / V tiles
// by LDS-DMA into a 3-slot ring; 64-key iterations; the INT32 QK^T accumulators start from the bit pattern of the inline constant
// 1 / (2 pi) = 0x3E22F983 (free as the MFMA's C operand), so read as a float they are 1 / (2 pi) + s * 2^-26 exactly and one exact v_add_f32
// replaces v_cvt_f32_i32; software-pipelined steady-state loops for FP8 and FP16 PV with their instruction order pinned in asm; FP8 PV on
// v_mfma_f32_32x32x64_f8f6f4; two-level requests accumulate P.V through the MFMA's FP32 C operand and rescale O only where a row maximum of
// the wave moved; the ticket loop in the non-causal kernels and in the packed route's causal ones.
#ifndef SAGE_ABL             // timing ablations of the FP8 pipelined loop (WRONG results; tools/build_variants.sh): 1 no O rescale, 2 no s_nop in
#define SAGE_ABL 0           // front of the loop's MFMAs (since they were dropped: 2 = WITH them), 4 no per-tile barrier, 8 no row-maximum chain, 16 no exponentials (v_mov instead), 32 no wait for the next tile's LDS-DMA at the top of a body
#endif
#ifndef SAGE_DIAG_PIPE       // causal FP8 D = 128: a work item's last two tiles through the pipelined body (1) or as general iterations (0: A/B)
#define SAGE_DIAG_PIPE 1
#endif
#ifndef SAGE_KARG_PREFETCH   // one scalar load per line of the parameter block at kernel entry (1) or not (0: A/B)
#define SAGE_KARG_PREFETCH 1
#endif
#ifndef SAGE_TAIL_PIPE       // non-causal FP8: the last two whole tiles (+ a ragged one behind them) through the pipelined body (1) or as general iterations (0: A/B)
#define SAGE_TAIL_PIPE 1
#endif
#ifndef SAGE_KSEL            // pipelined loops, per-thread k scale groups: the lane halves' scale products under EXEC (1) or by select (0: A/B)
#define SAGE_KSEL 1
#endif
#ifndef SAGE_ATTN_TRACE      // tools/attn_trace.py: wave 0 of every workgroup records 100 MHz time stamps of its phases
#define SAGE_ATTN_TRACE 0    // (entry, geometry known, Q ready, first tile landed, key loop done, epilogue barrier, stores issued, stores acknowledged)
#endif

// asm text of the pipelined loops: two scores d0 / d1 from the bit patterns s0 / s1 of the QK^T accumulators, d = score * c - m (operands as
// asm placeholders).  EXACT: the bias of the bit pattern is subtracted first (exact), then the FMA; FOLD (the FP8 opt-in variant): one FMA per
// score, m already carries the bias
#define SAGE_SCALE2_FOLD(d0, d1, s0, s1, c0, c1, m) "v_fma_f32 " d0 ", " s0 ", " c0 ", -" m "\n\tv_fma_f32 " d1 ", " s1 ", " c1 ", -" m "\n\t"
#define SAGE_SCALE2_EXACT(d0, d1, s0, s1, c0, c1, m) "v_add_f32 " d0 ", 0xbe22f983, " s0 "\n\tv_add_f32 " d1 ", 0xbe22f983, " s1 "\n\t" \
                                                      "v_fma_f32 " d0 ", " d0 ", " c0 ", -" m "\n\tv_fma_f32 " d1 ", " d1 ", " c1 ", -" m "\n\t"

// The pipelined loops' rename of the score tiles, set B -> set A (sA, sB: v16i[2] in scope), behind a body whose last instructions are the
// asm-issued MFMAs that write sB.  Plain copies (sA = sB) are moves the compiler is free to place right behind that asm -- inside the MFMAs'
// latency, which it does not see (round 5's wrong rows; an in-out nop statement in front of the copies does not help: the allocator may
// satisfy its tie by copying first).  So the copy is issued from asm as well, on the matrix pipe: D = 0 * 0 + C moves sixteen registers per
// instruction, exactly (INT32), behind the wait states an MFMA reading another MFMA's result as SrcC needs, and followed by those a VALU
// reader of its own result needs (tools/mfma_hazard_lint.py checks both).
#define SAGE_RENAME_S() do { const v4i z4_ = {0, 0, 0, 0};                                                                   \
        asm volatile("s_nop 15\n\ts_nop 7\n\tv_mfma_i32_32x32x32_i8 %0, %2, %2, %3\n\tv_mfma_i32_32x32x32_i8 %1, %2, %2, %4\n\t"     \
                     "s_nop 15\n\ts_nop 7" : "=&v"(sA[0]), "=&v"(sA[1]) : "v"(z4_), "v"(sB[0]), "v"(sB[1])); } while (0)

namespace sage {

// hwreg(HW_REG_MODE, 23, 1): the FP16_OVFL bit of the MODE register (id 1 | offset 23 << 6 | (width 1 - 1) << 11)
constexpr int kHwregModeFp16Ovfl = 1 | (23 << 6) | (0 << 11);


template <int D, bool PV_FP8, int NH> struct TileCfg {
    static constexpr int KT = BLKK * NH;                        // keys per iteration
    static constexpr int K_TILE_BYTES = KT * D;                 // int8
    static constexpr int V_ROW_BYTES = PV_FP8 ? 64 : 128;       // one 64-key image row
    static constexpr int V_IMG_BYTES = D * V_ROW_BYTES;
    static constexpr int STAGE_BYTES = K_TILE_BYTES + NH * V_IMG_BYTES;
    static constexpr int O_BYTES = BLKQ * D * 2;
    static constexpr int NSTAGE = 3;                            // LDS ring depth: two tiles in flight, counted vmcnt + raw s_barrier
    static constexpr int LDS_BYTES = (NSTAGE * STAGE_BYTES > O_BYTES) ? NSTAGE * STAGE_BYTES : O_BYTES;
    static constexpr int KSTEPS = D / 32;                       // i8 MFMA k-steps over head dim
    static constexpr int DT = D / 32;                           // 32-wide output d tiles
};

// c/d register r of a 32x32 MFMA tile -> row index inside the tile (lane half g = lane>>5)
__device__ __forceinline__ int crow(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }

// raw QK^T accumulator -> float score (in units of 2^-kSUnitLog2).
// 0x3E22F983 lies mid-binade ([0.125, 0.25), ulp 2^-26, mantissa field 2292099): for |s| <= 128 * 128 * 128 = 2097152 the sum
// stays inside the binade, so bits + s is the float 1/(2 pi) + s * 2^-26, the subtraction below is exact (Sterbenz) and
// fma(s * 2^-26, c * 2^26, -m) rounds the same real number as fma((float)s, c, -m): bit-identical to the conversion.
constexpr int kSUnitLog2 = 26;              // 2^26 is folded into the score scale -- by v_ldexp_f32 (exact, as a multiplication by 2^26 is, and the
                                            // exponent is an inline operand: the constant 2^26 in a VGPR was one the D = 64 instantiations spilled)
__device__ __forceinline__ float sfl(int x) { return __int_as_float(x) - __int_as_float(0x3E22F983); }
// first MFMA of a QK^T accumulation chain: C = kSInit as an inline constant (hipcc materialises an integer splat of
// 0x3E22F983 in 16 VGPRs instead; the assembler encodes it as inline operand 248).  The builtin MFMAs that follow take the
// result whole as their C operand (accumulate chain: no wait states, cdna_hip_programming.md 5.7 item 2).
__device__ __forceinline__ v16i mfma_i8_first(v4i a, v4i b)
{
    v16i d;
    asm("s_nop 1\n\tv_mfma_i32_32x32x32_i8 %0, %1, %2, 0x3e22f983" : "=&v"(d) : "v"(a), "v"(b));
    return d;
}

#if SAGE_ATTN_TRACE
// (the stamps go to AttnParams::trace, a caller-owned buffer of 16 words per logical workgroup: 8 stamps, -, HW_ID, XCC_ID, blockIdx.x, query block --
//  SageLaunchAttr::trace / trace_wgs, read by trace builds only)
#define SAGE_TSTAMP(i) do { if (wave == 0) { unsigned long long t_; \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); ttrace[i] = (unsigned)t_; } } while (0)
#else
#define SAGE_TSTAMP(i) do { } while (0)
#endif

// QF: 0 = q is INT8 with scales in q_scale; 1 / 2 = q is fp16 / bf16 and is quantised in the prologue, per-thread groups;
// 3 / 4 = fp16 / bf16 quantised in the prologue PER BLOCK of 128 rows after the multiplication by p.q_premul (quant_per_block.py:21-46
// with sm_scale folded in: the Q half of the reference's Triton-named API and of sageattn_varlen),
// ("per-thread" groups, quant_per_thread.py:21-52), so the INT8 copy of Q and its scales never touch HBM.
// SFOLD (FP8 PV only): false = the exact score form, exp2(fma(s, c, -m)) with the bias of the score's bit pattern subtracted first -- the
// reference's formula (attn_utils.cuh:445-449), the default of every entry point; true = the opt-in variant SAGE_ATTR_FP8_FOLDED_SCORES, the bias
// folded into the scale FMA in every tile of the launch (exp2(fma(bits, c', -(m + bias c'))): one VALU instruction less per score, m + bias c'
// rounded once per (row, tile, k scale); the oracle's score_mode 1 mirrors it).  FP16-PV instantiations have one form, the exact one, and pass true.
// CPERS: the persistent ticket loop compiled into a CAUSAL instantiation (the packed route's launches over the work list; non-causal unmasked
// instantiations always carry it).
// VROWS (FP16 PV, dense): p.v is the caller's fp16 V tensor itself, rows of D halves with element strides p.v_sb / v_sh / v_sl -- what the
// reference's kernels take (value fp16, last dimension contiguous: qk_int_sv_f16_cuda_sm80.cu:693-704) -- instead of the pre-transposed tile
// image of sage_prep_v_f16 / sage_prepass_kv.  A 64-token tile lands in LDS as rows (LDS-DMA through per-lane source addresses, like K) and
// the PV MFMA's A operand -- V^T: lane = channel, 8 tokens -- comes out of two transposing reads, ds_read_b64_tr_b16, which hand lane i of a
// 16-lane group element (i & 3) of the four 8-byte chunks that lanes (i >> 2), 4 + (i >> 2), 8 + .., 12 + .. address
// (tools/microbench/ubench9_tr_b16.hip, profiles/r6_run_c_ubench9_tr_b16.txt).  For fp16 inputs the V half of the pre-pass -- 2/3 of its
// bytes on an FP16-PV call -- disappears; the outputs are bit-identical to the image route's (same operands, same MFMAs).
// SEED (FP8 PV, fused per-thread Q, exact score form: pass 2 of the exact split-KV route, units sage_attn_d{128,64}_f8s.hip): launch head
// hk = hk0 * kv_split + chunk runs keys p.kv_base + chunk * Lk .. + Lk - 1 of kv head hk0 (the operands of the UNSPLIT call, read in place), its
// running maximum starts from the exclusive prefix maximum of pass 1's chunk maxima (p.seed_max) -- the maximum the unsplit call holds at the
// chunk's first tile, so every P is the unsplit call's -- and it writes an FP32 normalised partial output [B, Hq * kv_split, Lq, D].
// KVLEN (FP8 PV, fused per-thread Q, exact score form, dense: the kv_lens route, units sage_attn_d{128,64}_f8k.hip): sample b attends to keys
// 0 .. len_b - 1 only, len_b = p.cu_k[b] clamped to [0, p.Lk] (a dense launch leaves cu_k free; here it is the caller's [B] lengths).  Lk becomes
// len_b for everything that bounds, clamps or masks -- the work item then runs exactly what a call on the sample's first len_b keys runs --
// while what describes the TENSORS (V images and k scale slots per head) stays derived from the padded p.Lk.  Key rows, scales and V images
// from len_b on are never read.  A sample without keys requests no tile and runs no iteration (n_iters = 0); the epilogue then writes o = 0
// (l = 0: the normalisation factor is 0, and the product is forced to zero so that a NaN in the sample's unused scale slots cannot reach it)
// and lse = log2(0) + m = -inf.  (An exit of its own in front of the Q fragments -- a second way out of the item loop -- cost the D = 64
// non-causal instantiations 5-8 spilled VGPRs under their three-waves limit wherever it was placed.)
// QSTART (a CAUSAL KVLEN kernel, units sage_attn_d{128,64}_f8q.hip): query row 0 of sample b stands at key position s_b = p.cu_qs[b] clamped to
// [-p.Lq, p.Lk] (cu_qs is as free in a dense launch as cu_k), so row i attends to key j iff j <= s_b + i and j < len_b: s_b = 0 is the top-left
// mask, s_b = len_b - Lq the bottom-right one.  It is the split routes' shift of the causal mask into a chunk's key coordinates with
// kchunk0 = -s_b; loop bounds, the steady tiles and every mask follow from that value.  An offset that is a multiple of 64 keeps the pipelined
// last-tile bodies on the diagonal; any other puts the diagonal of a query block across three tiles, which run as general iterations
// (correct, slower).  A row with s_b + i < 0 sees nothing: every score of it is masked in every tile its wave runs, its maximum stays at
// kNegBig and its l at 0, and the epilogue gives it o = +0, lse = -inf as it does for a chunk of the inexact causal split that lies wholly
// behind a row's diagonal.
// QSTART without KVLEN (a CAUSAL packed launch, FP8 PV, per-block Q, two-level: units sage_attn_d{128,64}_f8vb.hip) is the packed route's
// bottom-right alignment: p.cu_q != null, and the offset of sequence b is s_b = Lk_b - Lq_b, formed from the four cu_seqlens words the packed
// branch has just loaded -- no operand of its own.  Everything above follows from kchunk0 = -s_b as it does for the dense kernels; a query block
// wholly in front of key 0 (lim = 0) and every block of a sequence without keys run no tile and write o = +0, lse = -inf.
// WINDOW (a QSTART kernel, units sage_attn_d{128,64}_f8w.hip): row i additionally sees only the last W = p.window keys up to its diagonal, s_b + i - W < j <= s_b + i.
// A work item starts at the 64-key tile that holds the first key its first row sees (kc0: k_off, v_tile0 and ks_ptr shifted as the SEED branch
// shifts them, Lk and kchunk0 in the shifted coordinates, so that loop bounds, steady tiles and masks follow as they do for QSTART) -- the tiles
// in front of it are never requested.  Its first `nh` tiles (at most three) are those in which some row of the block is cut on the left: they run
// as general iterations with one more comparison, in ascending key order, and behind them the ring is drained and primed again so that the
// pipelined loop is entered as ever, with its first tile in slot 0.  p.cu_qs may be null (offsets 0).  s_b is clamped to [-p.Lq, p.Lk + W]: a
// clamp to p.Lk would move the LEFT edge of an offset beyond the keys, which must see nothing.  With W >= p.Lk + p.Lq no row is cut, kc0 = 0 and
// nh = 0: the work item runs what the QSTART kernel runs.
// WINDOW with QSTART and without KVLEN (units sage_attn_d{128,64}_f8vbw.hip) is the packed bottom-right form with a window: s_b = Lk_b - Lq_b as
// above, W = p.window, the same head tiles, second priming and masks; only the shift of the item's first key is written for the packed layouts
// (V images and per-block k scales: one per 64-key tile, stride Hkv).  With the ticket loop (CPERS) the next item's ticket is requested behind
// the LAST tile of the item whichever run that is -- the request stands behind the remainder loop, not inside a run.
// GPACK (a KVLEN kernel, with or without QSTART / WINDOW; units sage_attn_d{128,64}_f8g.hip): a decode-shaped call (p.Lq <= 32) packs the query heads of a GQA group four to a workgroup.  A work
// item is (batch b, kv head hk, group block gb); wave w serves query head hk * group + 4 gb + w and takes rows 0 .. Lq - 1 of that head as the
// rows of its 32-row slab (row0 = 0 in every wave).  The head index and what follows from it alone -- q_off, o_off, the lse index -- are
// per wave (wave-uniform: SGPRs); everything else is what block 0 of the unpacked call forms from qblk = 0: the loop bounds, the head tiles,
// diag_ok / tail_ok, the tile requests, the barriers, the length / offset / window loads.  So wave w runs, instruction for instruction and on
// the same LDS contents, what wave 0 of its head's unpacked work item runs: the same bits.  A wave past the group's last
// head (4 gb + w >= group) is idle: it takes part in the tile requests and every barrier, loads no Q row (zeros, as rows past Lq are) and
// stores nothing; its head index is the group's first, so that no address is formed from a head past Hq.  No ticket loop: a decode launch
// does not reach twelve rounds of workgroups.
// SEED with KVLEN (non-causal, or causal with QSTART; with or without GPACK: units sage_attn_d{128,64}_f8ks.hip) is pass 2 of the kv_lens family's
// exact split (num_splits=): a call of one query block (p.Lq <= 128) as p.kv_split chunks of p.kv_base = 64 T keys, the chunk folded
// into the kv-head dimension as above.  A work item forms len_b and s_b as the KVLEN / QSTART kernels do and shifts both into its chunk: its
// first key is kc0 = chunk * 64 T, Lk becomes clamp(len_b - kc0, 0, 64 T) and kchunk0 = kc0 - s_b, so the loop bounds, the last-tile bodies and
// every mask are those of a call on the chunk's keys; the ragged last tile of a sample is simply the last tile of its last non-empty chunk.
// The running maximum starts from the prefix maximum of pass 1's chunk maxima and the FP32 normalised partial and its log2-domain LSE are
// stored per chunk; a chunk that holds no visible key -- past len_b, behind the block's diagonal, of an empty sample -- requests no tile and
// gives o = +0, lse = -inf, the weight 0 of the merge.
// FORM: pack() of the kernel's AttnForm (sage_attn_form.h), which also holds the rules on which flags may meet, on the waves per SIMD the
// register allocator must allow and on which kernels carry the ticket loop.
// RAGGED (sage_attn_paged_varlen_kernel below, a PAGED kernel of a causal QSTART form): packed query rows behind a prefix array -- not a form bit either.
// PAGED (sage_attn_paged_kernel below; a KVLEN kernel without SEED: DESIGN.md 3.18): K, the V image and the K scales are a POOL of pages of
// 64 << page_shift keys, laid out as the tensors of a call with B = num_pages and Lk = the page size, and logical 64-key tile t of sample b lies
// in page block_table[b][t >> page_shift] at tile t & (2^page_shift - 1) of it.  Not a form bit: the paged kernel of form F is form F with its
// tile addresses -- k_tile / v_tile / ks_slot of sage_attn_body.h, the only places that form one -- going through the table.  p.Lk is the logical capacity
// (pages per sequence * page size) and bounds, clamps and masks as ever; p.nks the scale slots of ONE page.  A page id is read with a scalar
// load (wave-uniform index, constant address space) and clamped to [0, num_pages - 1] before it forms an address; only the entries of tiles
// that hold a key the item requests are read.
template <uint32_t FORM>
__global__ void __launch_bounds__(256, min_waves(unpack(FORM)))
sage_attn_kernel(const AttnParams p_arg)
{
#define SAGE_ATTN_BODY_PAGED false
#define SAGE_ATTN_BODY_RAGGED false
#define SAGE_ATTN_BODY_BAND false
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_BAND
#undef SAGE_ATTN_BODY_RAGGED
#undef SAGE_ATTN_BODY_PAGED
}

// form FORM, tiles through a block table: the same body, the paged operands as a second argument behind the unchanged parameter block.
// (The body is shared as TEXT, the way the pipelined loops are: called as a __forceinline__ function template it gave the existing kernels another
//  register allocation -- 31 000 differing lines in sage_attn_d64_f8k.s -- where the included fragment gives their listings byte for byte.)
template <uint32_t FORM>
__global__ void __launch_bounds__(256, min_waves(unpack(FORM)))
sage_attn_paged_kernel(const AttnParams p_arg, const PagedArgs g_arg)
{
    (void)g_arg;
#define SAGE_ATTN_BODY_PAGED true
#define SAGE_ATTN_BODY_RAGGED false
#define SAGE_ATTN_BODY_BAND false
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_BAND
#undef SAGE_ATTN_BODY_RAGGED
#undef SAGE_ATTN_BODY_PAGED
}

// the paged kernel of form FORM (causal with QSTART: the q_start / window forms) over PACKED query rows: q / o [total_q, Hq, D], lse [Hq, total_q],
// sample b's rows cu_q[b] .. cu_q[b + 1] - 1.  The ragged operands are a third argument behind the two unchanged ones.  A work
// item is the dense one, (b, h, qblk) over nqblk = ceil(max_seqlen_q / 128) blocks; its prologue reads and clamps the two prefix words
// (ragged_rows, sage_ragged.h), takes Lq, q_off and o_off from them and leaves when the block lies past the sample's last row -- from there on
// it runs what the paged kernel runs for a call of that sample's own Lq, and its LSE goes to the packed route's index.  The form's own
// launch bound holds: the new state is wave-uniform (SGPRs), the eight kernels take 158 - 168 VGPRs at D = 64 and 232 - 238 at D = 128, no scratch.
template <uint32_t FORM>
__global__ void __launch_bounds__(256, min_waves(unpack(FORM)))
sage_attn_paged_varlen_kernel(const AttnParams p_arg, const PagedArgs g_arg, const RaggedArgs r_arg)
{
    (void)g_arg;
    (void)r_arg;
#define SAGE_ATTN_BODY_PAGED true
#define SAGE_ATTN_BODY_RAGGED true
#define SAGE_ATTN_BODY_BAND false
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_BAND
#undef SAGE_ATTN_BODY_RAGGED
#undef SAGE_ATTN_BODY_PAGED
}

// the ragged paged kernel of form FORM behind a BAND filter: one launch of the step call (include/sage_kvstep_gfx950.h).  The band's
// two words are a fourth argument behind the three unchanged ones; a work item whose sample's clamped row count lies outside (lo, hi] leaves where
// a query block past the sample's last row leaves (ragged_band, sage_ragged.h), every other item runs what sage_attn_paged_varlen_kernel<FORM>
// runs.  Instantiated for the forms of the ragged units -- the chunk launch, band (32, max_seqlen_q], the ragged launch's grid and work order --
// and for the QSTART forms of the packed-group list -- the decode launch, band (0, 32]: GPACK's own work item (b, kv head, block of four query
// heads), each wave taking the sample's <= 32 packed rows of its own head, so a decode sequence streams its K / V once per four heads.
template <uint32_t FORM>
__global__ void __launch_bounds__(256, min_waves(unpack(FORM)))
sage_attn_paged_step_kernel(const AttnParams p_arg, const PagedArgs g_arg, const RaggedArgs r_arg, const BandArgs b_arg)
{
    (void)g_arg;
    (void)r_arg;
    (void)b_arg;
#define SAGE_ATTN_BODY_PAGED true
#define SAGE_ATTN_BODY_RAGGED true
#define SAGE_ATTN_BODY_BAND true
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_BAND
#undef SAGE_ATTN_BODY_RAGGED
#undef SAGE_ATTN_BODY_PAGED
}

}  // namespace sage
