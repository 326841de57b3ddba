// sage_attn_d64_f8p.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_paged_units<64, SAGE_PAGED_UNITS>
// (the paged kernels, sage_attn_paged_kernel<FORM>: the kv_lens / q_start / window kernels with their tiles reached through a block table)
#include "sage_attn_launch.h"
#include "sage_attn_parts.h"
namespace sage {
template hipError_t launch_attn_paged_units<64, SAGE_PAGED_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, int, const AttnLaunchOpts &);
}
