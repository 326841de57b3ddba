// sage_attn_d64_f16.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F16, 64>
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F16, 64>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
