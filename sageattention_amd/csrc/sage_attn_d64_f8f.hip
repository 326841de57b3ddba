// sage_attn_d64_f8f.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F8F, 64>
// (FP8 PV, the folded score form: the opt-in variant SAGE_ATTR_FP8_FOLDED_SCORES)
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F8F, 64>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
