// sage_attn_d128_f8s.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F8S, 128>
// (the exact split-KV route's pass 2: fused per-thread Q, FP8 PV two-level, exact score form, seeded running maximum, FP32 partials)
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F8S, 128>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
