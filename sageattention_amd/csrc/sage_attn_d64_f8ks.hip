// sage_attn_d64_f8ks.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F8KS, 64>
// (the num_splits route's pass 2: the kv_lens / q_start kernels, unpacked and with packed GQA groups, over one key-range chunk each, seeded
// running maximum, FP32 partials)
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F8KS, 64>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
