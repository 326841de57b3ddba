// sage_attn_d64_f8.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F8, 64>
// (FP8 PV, the exact score form: the default of every FP8 entry point)
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F8, 64>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
