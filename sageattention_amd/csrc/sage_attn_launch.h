// sage_attn_launch.h -- host side of the attention kernel family: the one launch path every instantiation takes (dynamic-LDS opt-in, the
// persistent / ticket route) and the map from a launch's variant to the instantiation of sage_attn_kernel.h that runs it.  Included by the
// instantiation units sage_attn_d{128,64}_{f8,f8f,f16}.hip behind the kernel header.
#pragma once
#include "sage_attn_kernel.h"
#include <atomic>

namespace sage {

// ---------------------------------------------------------------------------------------------
// One launch path for every instantiation.  KERN is a non-type template argument, so the statics below exist once per kernel: the
// > 64 KiB dynamic-LDS opt-in (hipFuncAttributeMaxDynamicSharedMemorySize) is issued once per kernel and device, and the number of
// workgroups the device holds of THIS kernel is probed once per kernel and device (both lock-free: a race repeats the idempotent probe).
constexpr int kPersistMinRounds = 12;

template <auto KERN>
static hipError_t launch_kernel(int lds, const AttnParams &p, int nwork, const AttnLaunchOpts &l, bool persist_ok)
{
    static std::atomic<unsigned long long> lds_done{0};      // bit per device ordinal (mod 64)
    static std::atomic<int> slots_of[64];                    // per device ordinal (mod 64): 0 = not probed yet, else 1 + resident workgroups
    int dev = -1;
    const bool dev_ok = hipGetDevice(&dev) == hipSuccess && dev >= 0;
    if (lds > 65536) {
        if (!dev_ok) return hipErrorInvalidDevice;
        const unsigned long long bit = 1ull << (dev & 63);
        if (!(lds_done.load(std::memory_order_relaxed) & bit)) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (e != hipSuccess) return e;
            lds_done.fetch_or(bit, std::memory_order_relaxed);
        }
    }
    AttnParams pp = p;
    int grid = nwork;
    // Persistent launch (AttnParams::sched, a zeroed counter block of the caller; non-causal unmasked kernels): as many workgroups as the
    // device holds at once take the logical workgroup indices 0 .. nwork - 1 from 32 ticket queues (see the kernel).  Worth it from twelve
    // rounds of workgroups up -- one item must be small against the few per cent the XCDs differ by, or nothing can be evened out: with
    // eight rounds of equal items (B2 H32 N8192 non-causal) the tickets cost 1 % -- anything else is an ordinary launch.
    // What the route NEEDS (checked here, else the ordinary launch): the grid a multiple of 32 (the first round then covers whole tickets of
    // every queue) and not larger than the logical grid (every first-round workgroup has an item).  What it merely ASSUMES, for speed only:
    // blockIdx.x & 7 = the XCD of a first-round workgroup, and that the grid is co-resident (an unpartitioned 256-CU device, no CU mask).  On a
    // partitioned device or a CU-masked stream every logical index is still taken exactly once (tests/test_work_order.py restates the
    // partition); the queues then no longer match the L2s.  A failing occupancy probe is not an error of the call: ordinary launch.
    if (pp.sched != nullptr) {
        unsigned *sched = pp.sched;
        pp.sched = nullptr;
        if (persist_ok && dev_ok && (nwork & 7) == 0) {
            int slots = slots_of[dev & 63].load(std::memory_order_relaxed) - 1;
            if (slots < 0) {
                int ncu = 0, per_cu = 0;
                if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
                    hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(KERN), 256, lds) == hipSuccess)
                    slots = ncu * per_cu;
                else {
                    slots = 0;
                    (void)hipGetLastError();
                }
                slots_of[dev & 63].store(slots + 1, std::memory_order_relaxed);
            }
            const bool rounds_ok = l.force_persistent ? nwork >= 2 * slots : nwork >= kPersistMinRounds * slots;
            if (slots > 0 && (slots & 31) == 0 && rounds_ok) { pp.sched = sched; pp.nwg = nwork; grid = slots; }
        }
    }
    if (l.grid_out != nullptr) *l.grid_out = grid;
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(256), lds, l.stream, pp);
    return hipGetLastError();
}

// The members of the family one instantiation unit holds: INT8 q (8 of causal x k-scale groups x accumulation), the fused per-thread Q
// quantiser (fp16 / bf16 q), and for FP16 PV the masked kernels and the fused per-block Q quantiser.
// Keys per iteration: 64 (NH = 1).
// These launchers are called by launch_attention (sage_attn.hip) alone, after its route_exists(): they match a variant to its instantiation
// and refuse (hipErrorInvalidValue) only what no instantiation of the unit matches.
template <int D, bool PV_FP8, bool SFOLD>
hipError_t launch_attn_part(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l)
{
    static_assert(PV_FP8 || SFOLD, "FP16 PV has one score form");
    constexpr int NH = 1;
    using C = TileCfg<D, PV_FP8, NH>;
    // causal launches take the ticket route only over a packed batch's work list (items of very different lengths, heaviest first: +2.9 % at
    // C4), in instantiations of their own (CPERS); dense causal launches keep the hardware's dispatch, which their work order is built on
    const bool packed_list = p.cu_q != nullptr && p.work_items != nullptr;
    const bool pers = !v.causal;
    if (v.mask_kind != 0) {       // Triton-named API: FP16 PV, per-block scales, non-causal, tile product folded into the FP32 output
        if constexpr (!PV_FP8) {
            using CM = TileCfg<D, false, 1>;
            if (v.mask_kind == 1) return launch_kernel<sage_attn_kernel<D, false, false, false, true, 1, 1>>(CM::LDS_BYTES, p, nwork, l, false);
            if (v.mask_kind == 2) return launch_kernel<sage_attn_kernel<D, false, false, false, true, 1, 2>>(CM::LDS_BYTES, p, nwork, l, false);
            if (v.mask_kind == 3) return launch_kernel<sage_attn_kernel<D, false, false, false, true, 1, 3>>(CM::LDS_BYTES, p, nwork, l, false);
        }
        return hipErrorInvalidValue;
    }
    if (p.v_rows != 0) {                   // V rows read in place (fp16 V, FP16 PV, dense): fused Q quantisation per thread group / per block, or INT8 q
        if constexpr (!PV_FP8) {
#define SAGE_VR(C_) \
            if (v.causal == C_ && v.qf == 1) return launch_kernel<sage_attn_kernel<D, false, C_, true, false, NH, 0, 1, false, true, false, true>>(C::LDS_BYTES, p, nwork, l, pers); \
            if (v.causal == C_ && v.qf == 3) return launch_kernel<sage_attn_kernel<D, false, C_, false, true, NH, 0, 3, false, true, false, true>>(C::LDS_BYTES, p, nwork, l, pers);
            SAGE_VR(false) SAGE_VR(true)
#undef SAGE_VR
            // INT8 q with its scales (ABI 21, sage_attn_qk_int8_pv_f16_vrows): the reference's native FP16-PV ops as they are -- query / key INT8,
            // value fp16 rows (pybind_sm80.cpp:21-27; the Triton forward, attn_qk_int8_per_block.py:130) -- in every k-scale grouping and both kernel forms
#define SAGE_VR0(C_, K_, T_) if (v.qf == 0 && v.causal == C_ && v.kthread == K_ && v.two_level == T_) \
            return launch_kernel<sage_attn_kernel<D, false, C_, K_, T_, NH, 0, 0, false, true, false, true>>(C::LDS_BYTES, p, nwork, l, pers);
            SAGE_VR0(false, false, false) SAGE_VR0(false, false, true) SAGE_VR0(true, false, false) SAGE_VR0(true, false, true)
            SAGE_VR0(false, true, false)  SAGE_VR0(false, true, true)  SAGE_VR0(true, true, false)  SAGE_VR0(true, true, true)
#undef SAGE_VR0
        }
        return hipErrorInvalidValue;
    }
    if (v.qf == 1 || v.qf == 2) {      // per-thread groups quantised in the prologue; FP8 PV: two-level, FP16 PV: straight FP32 accumulation
#define SAGE_FQ(C_, F_) if (v.causal == C_ && v.qf == F_) return launch_kernel<sage_attn_kernel<D, PV_FP8, C_, true, PV_FP8, NH, 0, F_, false, SFOLD>>(C::LDS_BYTES, p, nwork, l, pers);
        SAGE_FQ(false, 1) SAGE_FQ(false, 2) SAGE_FQ(true, 1) SAGE_FQ(true, 2)
#undef SAGE_FQ
        return hipErrorInvalidValue;
    }
    if (v.qf == 3 || v.qf == 4) {      // per-block Q in the prologue: the Triton-named API's kernels (FP16 PV, per-block k scales), dense or varlen
        if constexpr (!PV_FP8) {
            if (v.causal && packed_list) {
                if (v.qf == 3) return launch_kernel<sage_attn_kernel<D, false, true, false, true, NH, 0, 3, false, true, true>>(C::LDS_BYTES, p, nwork, l, true);
                return launch_kernel<sage_attn_kernel<D, false, true, false, true, NH, 0, 4, false, true, true>>(C::LDS_BYTES, p, nwork, l, true);
            }
#define SAGE_FQB(C_, F_) if (v.causal == C_ && v.qf == F_) return launch_kernel<sage_attn_kernel<D, false, C_, false, true, NH, 0, F_>>(C::LDS_BYTES, p, nwork, l, pers);
            SAGE_FQB(false, 3) SAGE_FQB(false, 4) SAGE_FQB(true, 3) SAGE_FQB(true, 4)
#undef SAGE_FQB
        }
        return hipErrorInvalidValue;
    }
#define SAGE_CASE(C_, K_, T_) if (v.causal == C_ && v.kthread == K_ && v.two_level == T_) \
        return launch_kernel<sage_attn_kernel<D, PV_FP8, C_, K_, T_, NH, 0, 0, false, SFOLD>>(C::LDS_BYTES, p, nwork, l, pers);
    SAGE_CASE(false, false, false) SAGE_CASE(false, false, true)
    SAGE_CASE(true, false, false)  SAGE_CASE(true, false, true)
    SAGE_CASE(false, true, false)  SAGE_CASE(false, true, true)
    SAGE_CASE(true, true, false)   SAGE_CASE(true, true, true)
#undef SAGE_CASE
    return hipErrorInvalidValue;
}

// FP8 PV over a packed batch with the per-block Q quantiser in the prologue (qf 3 / 4: fp16 / bf16 q, sm_scale log2(e) folded into q), the
// exact score form, per-block k scales, two-level or single accumulation: the instantiation units sage_attn_d{128,64}_f8v.hip.  Causal
// launches over the device-built work list take the ticket route as the FP16 ones do (CPERS); without a work list the hardware's dispatch.
template <int D>
hipError_t launch_attn_f8_varlen(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l)
{
    using C = TileCfg<D, true, 1>;
    const bool pers = !v.causal;
    if (v.causal && p.work_items != nullptr) {
#define SAGE_F8VP(F_, T_) if (v.qf == F_ && v.two_level == T_) \
        return launch_kernel<sage_attn_kernel<D, true, true, false, T_, 1, 0, F_, false, false, true>>(C::LDS_BYTES, p, nwork, l, true);
        SAGE_F8VP(3, false) SAGE_F8VP(3, true) SAGE_F8VP(4, false) SAGE_F8VP(4, true)
#undef SAGE_F8VP
        return hipErrorInvalidValue;
    }
#define SAGE_F8V(C_, F_, T_) if (v.causal == C_ && v.qf == F_ && v.two_level == T_) \
    return launch_kernel<sage_attn_kernel<D, true, C_, false, T_, 1, 0, F_, false, false>>(C::LDS_BYTES, p, nwork, l, pers);
    SAGE_F8V(false, 3, false) SAGE_F8V(false, 3, true) SAGE_F8V(false, 4, false) SAGE_F8V(false, 4, true)
    SAGE_F8V(true, 3, false)  SAGE_F8V(true, 3, true)  SAGE_F8V(true, 4, false)  SAGE_F8V(true, 4, true)
#undef SAGE_F8V
    return hipErrorInvalidValue;
}

// The packed route with bottom-right causal alignment (sage_attn_kernel's QSTART without KVLEN: the offset of a sequence is Lk - Lq, formed from its
// cu_seqlens words): causal, FP8 PV two-level, the exact score form, per-block Q (qf 3 / 4), each as the ticket kernel (CPERS, over the work list)
// and as the plain one (no work list: the hardware's dispatch): the units sage_attn_d{128,64}_f8vb.hip.
template <int D>
hipError_t launch_attn_f8_varlen_br(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l)
{
    using C = TileCfg<D, true, 1>;
    if (!v.causal || !v.two_level) return hipErrorInvalidValue;
    const bool list = p.work_items != nullptr;
#define SAGE_F8VB(F_, P_) if (v.qf == F_ && list == P_) \
    return launch_kernel<sage_attn_kernel<D, true, true, false, true, 1, 0, F_, false, false, P_, false, false, false, true, false>>(C::LDS_BYTES, p, nwork, l, P_);
    SAGE_F8VB(3, true) SAGE_F8VB(3, false) SAGE_F8VB(4, true) SAGE_F8VB(4, false)
#undef SAGE_F8VB
    return hipErrorInvalidValue;
}

// The same route with a sliding window (sage_attn_kernel's WINDOW with QSTART and without KVLEN: p.window keys up to each row's bottom-right
// diagonal): the same four kernels per unit, the units sage_attn_d{128,64}_f8vbw.hip.
template <int D>
hipError_t launch_attn_f8_varlen_br_window(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l)
{
    using C = TileCfg<D, true, 1>;
    if (!v.causal || !v.two_level || !v.bottom_right || v.window <= 0) return hipErrorInvalidValue;
    const bool list = p.work_items != nullptr;
#define SAGE_F8VBW(F_, P_) if (v.qf == F_ && list == P_) \
    return launch_kernel<sage_attn_kernel<D, true, true, false, true, 1, 0, F_, false, false, P_, false, false, true, true, false>>(C::LDS_BYTES, p, nwork, l, P_);
    SAGE_F8VBW(3, true) SAGE_F8VBW(3, false) SAGE_F8VBW(4, true) SAGE_F8VBW(4, false)
#undef SAGE_F8VBW
    return hipErrorInvalidValue;
}

// The exact split's pass 2 (sage_attn_kernel's SEED): the fused per-thread Q quantiser (qf 1 / 2), FP8 PV two-level, the exact score form; the
// running maximum starts from pass 1's prefix maximum and the partial outputs are FP32: the units sage_attn_d{128,64}_f8s.hip.  Split launches
// take the hardware's dispatch (as the inexact split's do).
template <int D>
hipError_t launch_attn_f8_seeded(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l)
{
    using C = TileCfg<D, true, 1>;
#define SAGE_F8S(C_, F_) if (v.causal == C_ && v.qf == F_) \
    return launch_kernel<sage_attn_kernel<D, true, C_, true, true, 1, 0, F_, false, false, false, false, true>>(C::LDS_BYTES, p, nwork, l, false);
    SAGE_F8S(false, 1) SAGE_F8S(false, 2) SAGE_F8S(true, 1) SAGE_F8S(true, 2)
#undef SAGE_F8S
    return hipErrorInvalidValue;
}

// Per-sample key lengths (sage_attn_kernel's KVLEN): the fused per-thread Q quantiser (qf 1 / 2), FP8 PV two-level, the exact score form, dense;
// p.cu_k holds the [B] lengths: the units sage_attn_d{128,64}_f8k.hip.  Non-causal launches may take the ticket route as the plain kernels do
// (samples of different lengths are items of different lengths: the tickets even them out); causal launches keep the hardware's dispatch.
template <int D>
hipError_t launch_attn_f8_kvlens(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l)
{
    using C = TileCfg<D, true, 1>;
#define SAGE_F8K(C_, F_) if (v.causal == C_ && v.qf == F_) \
    return launch_kernel<sage_attn_kernel<D, true, C_, true, true, 1, 0, F_, false, false, false, false, false, false, false, true>>(C::LDS_BYTES, p, nwork, l, !C_);
    SAGE_F8K(false, 1) SAGE_F8K(false, 2) SAGE_F8K(true, 1) SAGE_F8K(true, 2)
#undef SAGE_F8K
    return hipErrorInvalidValue;
}

// Per-sample query offsets on top of the key lengths (sage_attn_kernel's QSTART): the causal kv_lens kernels with p.cu_qs = the [B] offsets:
// the units sage_attn_d{128,64}_f8q.hip.  The hardware's dispatch over the work order planned for the padded shapes, as every dense causal launch.
template <int D>
hipError_t launch_attn_f8_qstart(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l)
{
    using C = TileCfg<D, true, 1>;
#define SAGE_F8Q(F_) if (v.causal && v.qf == F_) \
    return launch_kernel<sage_attn_kernel<D, true, true, true, true, 1, 0, F_, false, false, false, false, false, false, true, true>>(C::LDS_BYTES, p, nwork, l, false);
    SAGE_F8Q(1) SAGE_F8Q(2)
#undef SAGE_F8Q
    return hipErrorInvalidValue;
}

// A sliding window on top of the query offsets (sage_attn_kernel's WINDOW): the q_start kernels with p.window keys per row, p.cu_qs nullable: the
// units sage_attn_d{128,64}_f8w.hip.  The hardware's dispatch over the causal work order planned for the padded shapes.
template <int D>
hipError_t launch_attn_f8_window(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l)
{
    using C = TileCfg<D, true, 1>;
#define SAGE_F8W(F_) if (v.causal && v.qf == F_) \
    return launch_kernel<sage_attn_kernel<D, true, true, true, true, 1, 0, F_, false, false, false, false, false, true, true, true>>(C::LDS_BYTES, p, nwork, l, false);
    SAGE_F8W(1) SAGE_F8W(2)
#undef SAGE_F8W
    return hipErrorInvalidValue;
}

// Packed GQA groups for decode-shaped calls (sage_attn_kernel's GPACK: p.Lq <= 32, the query heads of a group four to a workgroup, one wave
// each over one shared K / V ring): the kv_lens family's four members -- non-causal and causal lengths, query offsets, a window on top of
// them -- in units of their own, sage_attn_d{128,64}_f8g.hip.  The ordinary launch alone: the ticket loop is not compiled into these kernels
// (a decode launch of twelve rounds of workgroups does not occur, and the loop costs registers wherever it stands).
template <int D>
hipError_t launch_attn_f8_gpack(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l)
{
    using C = TileCfg<D, true, 1>;
    if (!v.gqa_pack || !v.kv_lens) return hipErrorInvalidValue;
    const bool window = v.window > 0, offsets = v.q_start || window;
#define SAGE_F8G(C_, F_, W_, Q_) if (v.causal == C_ && v.qf == F_ && window == W_ && offsets == Q_) \
    return launch_kernel<sage_attn_kernel<D, true, C_, true, true, 1, 0, F_, true, false, false, false, false, W_, Q_, true>>(C::LDS_BYTES, p, nwork, l, false);
    SAGE_F8G(false, 1, false, false) SAGE_F8G(false, 2, false, false) SAGE_F8G(true, 1, false, false) SAGE_F8G(true, 2, false, false)
    SAGE_F8G(true, 1, false, true)   SAGE_F8G(true, 2, false, true)   SAGE_F8G(true, 1, true, true)   SAGE_F8G(true, 2, true, true)
#undef SAGE_F8G
    return hipErrorInvalidValue;
}

// Pass 2 of the kv_lens family's exact split (sage_attn_kernel's SEED with KVLEN): the chunks of a call of one query block folded into the
// kv-head dimension, non-causal with lengths or causal with offsets (QSTART, p.cu_qs nullable), each unpacked and with packed GQA groups: the
// units sage_attn_d{128,64}_f8ks.hip.  The ordinary launch alone.
template <int D>
hipError_t launch_attn_f8_kvsplit(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l)
{
    using C = TileCfg<D, true, 1>;
    if (!v.seeded || !v.kv_lens || v.window != 0) return hipErrorInvalidValue;
#define SAGE_F8KS(C_, F_, G_) if (v.causal == C_ && v.qf == F_ && v.gqa_pack == G_) \
    return launch_kernel<sage_attn_kernel<D, true, C_, true, true, 1, 0, F_, G_, false, false, false, true, false, C_, true>>(C::LDS_BYTES, p, nwork, l, false);
    SAGE_F8KS(false, 1, false) SAGE_F8KS(false, 2, false) SAGE_F8KS(true, 1, false) SAGE_F8KS(true, 2, false)
    SAGE_F8KS(false, 1, true)  SAGE_F8KS(false, 2, true)  SAGE_F8KS(true, 1, true)  SAGE_F8KS(true, 2, true)
#undef SAGE_F8KS
    return hipErrorInvalidValue;
}

}  // namespace sage
