// sage_attn_d128_f8plg.hip -- instantiation unit of the attention kernel family (sage_attn_list_kernel.h): launch_attn_list_units<128, SAGE_STEP_G_UNITS>
// (the listed step call's decode launch: the QSTART forms of the packed-group list over the device-built decode list, sage_attn_paged_list_kernel<FORM>)
#include "sage_attn_list_kernel.h"
#include "sage_attn_parts.h"
namespace sage {
template hipError_t launch_attn_list_units<128, SAGE_STEP_G_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
}
