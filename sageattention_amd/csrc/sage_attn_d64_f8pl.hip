// sage_attn_d64_f8pl.hip -- instantiation unit of the attention kernel family (sage_attn_list_kernel.h): launch_attn_list_units<64, SAGE_STEP_UNITS>
// (the listed step call's chunk launch: the ragged paged q_start / window kernels over the device-built chunk list, sage_attn_paged_list_kernel<FORM>)
#include "sage_attn_list_kernel.h"
#include "sage_attn_parts.h"
namespace sage {
template hipError_t launch_attn_list_units<64, SAGE_STEP_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
}
