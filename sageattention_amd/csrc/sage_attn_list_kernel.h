// sage_attn_list_kernel.h -- the fifth entry over sage_attn_body.h: sage_attn_paged_list_kernel<FORM>, the step kernel of form FORM whose work
// items come from the device-built lists of sage_kv_list_plan.hip (include/sage_kvlist_gfx950.h).  A header of its own: the four
// entries of sage_attn_kernel.h and their switches stay what they are, and only the units sage_attn_d{128,64}_{f8pl,f8plg}.hip include this one
// (and, through sage_attn_lsplit_kernel.h, the units sage_attn_d{128,64}_f8plks.hip: the same entry over SEED forms).
//
// The arguments are the step kernel's, argument for argument -- the parameter block, the paged, the ragged and the band operands at their
// offsets; the lists travel in AttnParams::work_hdr / work_items, which a paged launch leaves free (AttnParams::cu_q stays null: the dense
// branches of the body).  What differs is the work-item site alone (LIST in the body):
//   chunk forms   work_hdr = {nitems, group, fold, left} and work_items = (sequence, query block) pairs, heaviest first: the launch is a dense
//                 launch over Hq heads of nitems "query blocks", dealt by work_item() as the packed route's list is; the grid is sized by
//                 AttnParams::items_bound, the workgroups past the header's count leave;
//   decode forms  work_hdr[0] = n_decode and work_items = the decode sequences, heaviest first: units (list rank, kv head) go to the XCDs
//                 round-robin, the ceil(group / 4) blocks of a unit stay on one XCD; grid 8 * ceil(B * Hkv / 8) * ceil(group / 4).
// Every list word is clamped before anything is formed from it.  The row-range site is the band arm verbatim: the prefix words are read again
// and ragged_band decides, so an item whose sequence lies outside the launch's band leaves there, and an item that stays runs instruction for
// instruction what sage_attn_paged_step_kernel<FORM>'s item runs -- the same bits.
#pragma once
#include "sage_attn_launch.h"

namespace sage {

template <uint32_t FORM>
__global__ void __launch_bounds__(256, min_waves(unpack(FORM)))
sage_attn_paged_list_kernel(const AttnParams p_arg, const PagedArgs g_arg, const RaggedArgs r_arg, const BandArgs b_arg)
{
    (void)g_arg;
    (void)r_arg;
    (void)b_arg;
#define SAGE_ATTN_BODY_PAGED true
#define SAGE_ATTN_BODY_RAGGED true
#define SAGE_ATTN_BODY_BAND true
#define SAGE_ATTN_BODY_LIST true
#include "sage_attn_body.h"
#undef SAGE_ATTN_BODY_LIST
#undef SAGE_ATTN_BODY_BAND
#undef SAGE_ATTN_BODY_RAGGED
#undef SAGE_ATTN_BODY_PAGED
}

// The list units: the list kernels of the QSTART forms of the named units' lists, through the one launch path (sage_attn_launch.h), as the step
// units' launcher walks them
template <uint32_t F>
static hipError_t launch_list_form(const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork, const AttnLaunchOpts &l)
{
    if constexpr (unpack(F).qstart)
        return launch_kernel<sage_attn_paged_list_kernel<F>>(TileCfg<unpack(F).D, unpack(F).pv_fp8, 1>::LDS_BYTES, p, nwork, l, false, g, r, b);
    else
        return hipErrorInvalidValue;
}

template <uint32_t... F>
static bool launch_list_among(Forms<F...>, uint32_t want, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork,
                              const AttnLaunchOpts &l, hipError_t &e)
{
    return ((want == F && ((e = launch_list_form<F>(p, g, r, b, nwork, l)), true)) || ...);
}

template <int D, AttnUnit... U>
hipError_t launch_attn_list_units(uint32_t form, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork, const AttnLaunchOpts &l)
{
    hipError_t e = hipErrorInvalidValue;
    (void)(launch_list_among(typename UnitForms<U, D>::type{}, form, p, g, r, b, nwork, l, e) || ...);
    return e;
}

}  // namespace sage
