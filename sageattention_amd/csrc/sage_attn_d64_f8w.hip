// sage_attn_d64_f8w.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F8W, 64>
// (the window_size route: the q_start kernels with a bounded look-back -- row i sees the last W keys up to its diagonal)
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F8W, 64>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
