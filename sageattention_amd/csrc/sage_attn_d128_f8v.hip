// sage_attn_d128_f8v.hip -- instantiation unit of the attention kernel family (sage_attn_kernel.h): launch_attn_unit<UNIT_F8V, 128>
// (FP8 PV over a packed batch, per-block Q quantised in the prologue, the exact score form: sage_attn_*_pv_f8_varlen)
#include "sage_attn_launch.h"
namespace sage {
template hipError_t launch_attn_unit<UNIT_F8V, 128>(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
}
