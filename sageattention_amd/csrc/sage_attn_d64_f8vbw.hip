// sage_attn_d64_f8vbw.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F8VBW, 64>
// (the packed FP8-PV route, bottom-right causal alignment, with a sliding window: row i of a sequence sees key j iff i + Lk - Lq - W < j <= i + Lk - Lq)
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F8VBW, 64>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
