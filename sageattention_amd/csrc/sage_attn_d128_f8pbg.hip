// sage_attn_d128_f8pbg.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_step_units<128, SAGE_STEP_G_UNITS>
// (the step call's decode launch: the QSTART forms of the packed-group list as sage_attn_paged_step_kernel<FORM>, packed rows of <= 32 per sample)
#include "sage_attn_launch.h"
#include "sage_attn_parts.h"
namespace sage {
template hipError_t launch_attn_step_units<128, SAGE_STEP_G_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
}
