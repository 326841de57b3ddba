// sage_attn_d128_f8pg.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_paged_units<128, SAGE_PAGED_G_UNITS>
// (the paged kernels, sage_attn_paged_kernel<FORM>: the pack_gqa kernels with their tiles reached through a block table)
#include "sage_attn_launch.h"
#include "sage_attn_parts.h"
namespace sage {
template hipError_t launch_attn_paged_units<128, SAGE_PAGED_G_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, int, const AttnLaunchOpts &);
}
