// sage_attn_d128_f16.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F16, 128>
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F16, 128>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
