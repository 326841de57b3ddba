// sage_attn_d128_f8pb.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_step_units<128, SAGE_STEP_UNITS>
// (the step call's chunk launch: the ragged paged q_start / window kernels behind a band filter, sage_attn_paged_step_kernel<FORM>)
#include "sage_attn_launch.h"
#include "sage_attn_parts.h"
namespace sage {
template hipError_t launch_attn_step_units<128, SAGE_STEP_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
}
