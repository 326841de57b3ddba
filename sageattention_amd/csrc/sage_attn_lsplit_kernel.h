// sage_attn_lsplit_kernel.h -- pass 2 of the SPLIT step call (include/sage_kvlsplit_gfx950.h): the list entry
// sage_attn_paged_list_kernel<FORM> (sage_attn_list_kernel.h) over the SEEDED packed-group forms.  No new __global__ entry and no new switch: a
// SEED form under the list entry is the body's LSPLIT (sage_attn_body.h), which differs from the listed decode launch in four sites --
//   the work item    units (decode-list rank, chunk, kv head), step_split_item (sage_step_list.h), the chunk folded into the kv heads as the
//                    dense split folds it; grid 8 * ceil(B * S * Hkv / 8) * ceil(group / 4);
//   the geometry     the SEED && KVLEN branch with the band arm's row range in it: Q from the packed rows, the offset clamped with the
//                    sample's own row count;
//   the seed read and the LSE store   index the dense split workspace, whose rows per (sequence, head) are AttnParams::lse_sh =
//                    min(max_seqlen_q, 32) -- a quantity of its own, where the dense split call has its Lq;
// and whose partial rows go where the seeded kernels put them, through AttnParams::o_sb / o_sh / o_sl (set by the entry for that workspace).
// Only the units sage_attn_d{128,64}_f8plks.hip include this header.
#pragma once
#include "sage_attn_list_kernel.h"

namespace sage {

// The split units: the list kernels of the QSTART + GPACK forms of the named unit's list (UNIT_F8KS: fp16 / bf16 q), through the one launch
// path.  The filter stands here, where the list is walked: the unit's other six forms have no meaning in a step call and get no kernel.
template <uint32_t F>
static hipError_t launch_lsplit_form(const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork, const AttnLaunchOpts &l)
{
    if constexpr (unpack(F).qstart && unpack(F).gpack && unpack(F).seed && unpack(F).kvlen)
        return launch_kernel<sage_attn_paged_list_kernel<F>>(TileCfg<unpack(F).D, unpack(F).pv_fp8, 1>::LDS_BYTES, p, nwork, l, false, g, r, b);
    else
        return hipErrorInvalidValue;
}

template <uint32_t... F>
static bool launch_lsplit_among(Forms<F...>, uint32_t want, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork,
                                const AttnLaunchOpts &l, hipError_t &e)
{
    return ((want == F && ((e = launch_lsplit_form<F>(p, g, r, b, nwork, l)), true)) || ...);
}

template <int D, AttnUnit... U>
hipError_t launch_attn_lsplit_units(uint32_t form, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork, const AttnLaunchOpts &l)
{
    hipError_t e = hipErrorInvalidValue;
    (void)(launch_lsplit_among(typename UnitForms<U, D>::type{}, form, p, g, r, b, nwork, l, e) || ...);
    return e;
}

}  // namespace sage
