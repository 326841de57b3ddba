// sage_attn_launch.h -- host side of the attention kernel family: the one launch path every instantiation takes (dynamic-LDS opt-in, the
// persistent / ticket route) and the launcher that finds a launch's form among the kernels of an instantiation unit.  Included by the
// instantiation units sage_attn_d{128,64}_*.hip.
#pragma once
#include "sage_attn_kernel.h"
#include <atomic>

namespace sage {

// ---------------------------------------------------------------------------------------------
// One launch path for every instantiation.  KERN is a non-type template argument, so the statics below exist once per kernel: the
// > 64 KiB dynamic-LDS opt-in (hipFuncAttributeMaxDynamicSharedMemorySize) is issued once per kernel and device, and the number of
// workgroups the device holds of THIS kernel is probed once per kernel and device (both lock-free: a race repeats the idempotent probe).
constexpr int kPersistMinRounds = 12;

// (extra: kernel arguments behind the parameter block -- the paged kernels' PagedArgs)
template <auto KERN, class... Extra>
static hipError_t launch_kernel(int lds, const AttnParams &p, int nwork, const AttnLaunchOpts &l, bool persist_ok, const Extra &...extra)
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
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(256), lds, l.stream, pp, extra...);
    return hipGetLastError();
}

// The one launcher of every instantiation unit: the unit's list of forms (UnitForms<U, D>, sage_attn_form.h) instantiates its kernels, and the
// entry equal to the wanted form -- attn_form() of the launch, packed -- is launched with what follows from the form: the LDS bytes of its tile
// configuration and persist_ok.  Called by launch_attention (sage_attn.hip) alone, after its route_exists(); a form the unit does not hold is
// refused (hipErrorInvalidValue).  Each sage_attn_d{128,64}_<unit>.hip is one explicit instantiation of it.
template <uint32_t F>
static hipError_t launch_form(const AttnParams &p, int nwork, const AttnLaunchOpts &l)
{
    constexpr AttnForm f = unpack(F);
    return launch_kernel<sage_attn_kernel<F>>(TileCfg<f.D, f.pv_fp8, 1>::LDS_BYTES, p, nwork, l, persist_ok(f));
}

template <uint32_t... F>
static hipError_t launch_among(Forms<F...>, uint32_t want, const AttnParams &p, int nwork, const AttnLaunchOpts &l)
{
    hipError_t e = hipErrorInvalidValue;
    (void)((want == F && ((e = launch_form<F>(p, nwork, l)), true)) || ...);
    return e;
}

template <AttnUnit U, int D>
hipError_t launch_attn_unit(uint32_t form, const AttnParams &p, int nwork, const AttnLaunchOpts &l)
{
    return launch_among(typename UnitForms<U, D>::type{}, form, p, nwork, l);
}

// The paged units sage_attn_d{128,64}_{f8p,f8pg}.hip: the paged kernels (sage_attn_paged_kernel) of exactly the forms of the named units' lists --
// instantiated from those lists, nothing restated -- through the same launch path; never the ticket route (AttnParams::sched is ignored).
template <uint32_t... F>
static bool launch_paged_among(Forms<F...>, uint32_t want, const AttnParams &p, const PagedArgs &g, int nwork, const AttnLaunchOpts &l, hipError_t &e)
{
    return ((want == F && ((e = launch_kernel<sage_attn_paged_kernel<F>>(TileCfg<unpack(F).D, unpack(F).pv_fp8, 1>::LDS_BYTES, p, nwork, l, false, g)), true)) || ...);
}

template <int D, AttnUnit... U>
hipError_t launch_attn_paged_units(uint32_t form, const AttnParams &p, const PagedArgs &g, int nwork, const AttnLaunchOpts &l)
{
    hipError_t e = hipErrorInvalidValue;
    (void)(launch_paged_among(typename UnitForms<U, D>::type{}, form, p, g, nwork, l, e) || ...);
    return e;
}

// The ragged paged units sage_attn_d{128,64}_f8pr.hip: the ragged paged kernels (sage_attn_paged_varlen_kernel) of the forms of the named units'
// lists, as above; the ragged operands follow the paged ones behind the parameter block.
template <uint32_t... F>
static bool launch_ragged_among(Forms<F...>, uint32_t want, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, int nwork, const AttnLaunchOpts &l,
                                hipError_t &e)
{
    return ((want == F && ((e = launch_kernel<sage_attn_paged_varlen_kernel<F>>(TileCfg<unpack(F).D, unpack(F).pv_fp8, 1>::LDS_BYTES, p, nwork, l, false, g, r)), true)) || ...);
}

template <int D, AttnUnit... U>
hipError_t launch_attn_ragged_units(uint32_t form, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, int nwork, const AttnLaunchOpts &l)
{
    hipError_t e = hipErrorInvalidValue;
    (void)(launch_ragged_among(typename UnitForms<U, D>::type{}, form, p, g, r, nwork, l, e) || ...);
    return e;
}

// The step units sage_attn_d{128,64}_{f8pb,f8pbg}.hip: the step kernels (sage_attn_paged_step_kernel, the ragged paged kernels behind a band
// filter) of the QSTART forms of the named units' lists, as above; the band follows the ragged operands.  The filter stands here, where the list
// is walked: the packed-group list also holds four forms without offsets, which have no ragged meaning and get no kernel (nor a launch).
template <uint32_t F>
static hipError_t launch_step_form(const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork, const AttnLaunchOpts &l)
{
    if constexpr (unpack(F).qstart)
        return launch_kernel<sage_attn_paged_step_kernel<F>>(TileCfg<unpack(F).D, unpack(F).pv_fp8, 1>::LDS_BYTES, p, nwork, l, false, g, r, b);
    else
        return hipErrorInvalidValue;
}

template <uint32_t... F>
static bool launch_step_among(Forms<F...>, uint32_t want, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork,
                              const AttnLaunchOpts &l, hipError_t &e)
{
    return ((want == F && ((e = launch_step_form<F>(p, g, r, b, nwork, l)), true)) || ...);
}

template <int D, AttnUnit... U>
hipError_t launch_attn_step_units(uint32_t form, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork, const AttnLaunchOpts &l)
{
    hipError_t e = hipErrorInvalidValue;
    (void)(launch_step_among(typename UnitForms<U, D>::type{}, form, p, g, r, b, nwork, l, e) || ...);
    return e;
}

}  // namespace sage
