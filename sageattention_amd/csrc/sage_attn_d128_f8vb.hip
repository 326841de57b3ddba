// sage_attn_d128_f8vb.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F8VB, 128>
// (the packed FP8-PV route with bottom-right causal alignment: row i of a sequence sees key j iff j <= i + Lk - Lq; SAGE_ATTR_CAUSAL_BOTTOM_RIGHT)
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F8VB, 128>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
