// sage_attn_d64_f8g.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F8G, 64>
// (the pack_gqa route: the kv_lens / q_start / window kernels for decode-shaped calls, a GQA group's query heads four to a workgroup)
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F8G, 64>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
