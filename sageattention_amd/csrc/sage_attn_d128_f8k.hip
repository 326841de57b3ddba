// sage_attn_d128_f8k.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F8K, 128>
// (the kv_lens route: fused per-thread Q, FP8 PV two-level, exact score form, dense with a key length per sample)
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F8K, 128>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
