// sage_attn_parts.h -- interface between the host-side dispatch of the attention launches (sage_attn.hip) and the instantiation units
// sage_attn_d{128,64}_<unit>.hip, each of which compiles the kernels of one list of sage_attn_form.h (unit_forms) for one head size.  The split
// exists for build time only: the units are independent and compile in parallel.
#pragma once
#include "sage_attn_form.h"

namespace sage {

// launches the kernel of unit U whose packed form is `form` (sage_attn_launch.h); hipErrorInvalidValue if the unit holds none
template <AttnUnit U, int D>
hipError_t launch_attn_unit(uint32_t form, const AttnParams &p, int nwork, const AttnLaunchOpts &l);

#define SAGE_UNIT_EXTERN(U) \
    extern template hipError_t launch_attn_unit<UNIT_##U, 128>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &); \
    extern template hipError_t launch_attn_unit<UNIT_##U, 64>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
SAGE_ATTN_UNITS(SAGE_UNIT_EXTERN)
#undef SAGE_UNIT_EXTERN

// the paged kernels of the forms of units U... (sage_attn_launch.h): sage_attn_d{128,64}_f8p.hip holds those of F8K / F8Q / F8W,
// sage_attn_d{128,64}_f8pg.hip those of F8G; hipErrorInvalidValue if none of the lists holds `form`
template <int D, AttnUnit... U>
hipError_t launch_attn_paged_units(uint32_t form, const AttnParams &p, const PagedArgs &g, int nwork, const AttnLaunchOpts &l);
#define SAGE_PAGED_UNITS UNIT_F8K, UNIT_F8Q, UNIT_F8W
#define SAGE_PAGED_G_UNITS UNIT_F8G
#define SAGE_PAGED_KS_UNITS UNIT_F8KS      // sage_attn_d{128,64}_f8pks.hip: pass 2 of the kv_lens family's split on a paged cache
extern template hipError_t launch_attn_paged_units<128, SAGE_PAGED_KS_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_paged_units<64, SAGE_PAGED_KS_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_paged_units<128, SAGE_PAGED_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_paged_units<64, SAGE_PAGED_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_paged_units<128, SAGE_PAGED_G_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_paged_units<64, SAGE_PAGED_G_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, int, const AttnLaunchOpts &);

// the ragged paged kernels (packed query rows) of the forms of units U...: sage_attn_d{128,64}_f8pr.hip holds those of F8Q / F8W
template <int D, AttnUnit... U>
hipError_t launch_attn_ragged_units(uint32_t form, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, int nwork, const AttnLaunchOpts &l);
#define SAGE_RAGGED_UNITS UNIT_F8Q, UNIT_F8W
extern template hipError_t launch_attn_ragged_units<128, SAGE_RAGGED_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_ragged_units<64, SAGE_RAGGED_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, int, const AttnLaunchOpts &);

// the step kernels (the ragged paged kernels behind a band filter) of the QSTART forms of units U...: sage_attn_d{128,64}_f8pb.hip
// holds those of F8Q / F8W (the step call's chunk launch), sage_attn_d{128,64}_f8pbg.hip those of F8G (its decode launch)
template <int D, AttnUnit... U>
hipError_t launch_attn_step_units(uint32_t form, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork, const AttnLaunchOpts &l);
#define SAGE_STEP_UNITS UNIT_F8Q, UNIT_F8W
#define SAGE_STEP_G_UNITS UNIT_F8G
extern template hipError_t launch_attn_step_units<128, SAGE_STEP_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_step_units<64, SAGE_STEP_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_step_units<128, SAGE_STEP_G_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_step_units<64, SAGE_STEP_G_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);

// the list kernels (the step kernels over device-built work lists, sage_attn_list_kernel.h) of the QSTART forms of the same lists:
// sage_attn_d{128,64}_f8pl.hip holds those of F8Q / F8W (the listed step call's chunk launch), sage_attn_d{128,64}_f8plg.hip those of F8G (its decode launch)
template <int D, AttnUnit... U>
hipError_t launch_attn_list_units(uint32_t form, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork, const AttnLaunchOpts &l);
extern template hipError_t launch_attn_list_units<128, SAGE_STEP_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_list_units<64, SAGE_STEP_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_list_units<128, SAGE_STEP_G_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_list_units<64, SAGE_STEP_G_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);

// pass 2 of the split step call (the list kernels of the seeded packed-group forms, sage_attn_lsplit_kernel.h):
// sage_attn_d{128,64}_f8plks.hip holds those of the QSTART + GPACK forms of F8KS
template <int D, AttnUnit... U>
hipError_t launch_attn_lsplit_units(uint32_t form, const AttnParams &p, const PagedArgs &g, const RaggedArgs &r, const BandArgs &b, int nwork, const AttnLaunchOpts &l);
#define SAGE_STEP_KS_UNITS UNIT_F8KS
extern template hipError_t launch_attn_lsplit_units<128, SAGE_STEP_KS_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_lsplit_units<64, SAGE_STEP_KS_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);

}  // namespace sage
