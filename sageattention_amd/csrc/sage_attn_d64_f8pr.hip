// sage_attn_d64_f8pr.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_ragged_units<64, SAGE_RAGGED_UNITS>
// (the ragged paged kernels, sage_attn_paged_varlen_kernel<FORM>: the paged q_start / window kernels over packed query rows)
#include "sage_attn_launch.h"
#include "sage_attn_parts.h"
namespace sage {
template hipError_t launch_attn_ragged_units<64, SAGE_RAGGED_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, int, const AttnLaunchOpts &);
}
