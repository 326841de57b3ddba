// sage_attn_d64_f8q.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F8Q, 64>
// (the q_start route: the causal kv_lens kernels with a query offset per sample -- bottom-right causal alignment)
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F8Q, 64>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
