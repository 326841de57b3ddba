// sage_attn_d128_f8plks.hip -- instantiation unit of the attention kernel family (sage_attn_lsplit_kernel.h): launch_attn_lsplit_units<128, SAGE_STEP_KS_UNITS>
// (the split step call's pass 2: the QSTART + GPACK forms of the kv_lens split's list over the device-built decode list, sage_attn_paged_list_kernel<FORM>)
#include "sage_attn_lsplit_kernel.h"
#include "sage_attn_parts.h"
namespace sage {
template hipError_t launch_attn_lsplit_units<128, SAGE_STEP_KS_UNITS>(uint32_t, const AttnParams &, const PagedArgs &, const RaggedArgs &, const BandArgs &, int, const AttnLaunchOpts &);
}
