// sage_host_checks.h -- the argument checks of the C entry points, host code only (sage_cabi.hip, sage_kv_cache.hip, sage_kv_paged.hip, sage_kv_fork.hip): one
// require-or-fail macro over the library's error channel and the alignment / stride predicates.  No other unit includes it.
#pragma once
#include "../../include/sage_gfx950.h"
#include "sage_kernels.h"

#include <cstdint>

// `cond`, or the entry returns SAGE_EINVAL with the printf-style message that sage_last_error() then reports
#define SAGE_REQUIRE(cond, ...) do { if (!(cond)) return sage::set_last_error(SAGE_EINVAL, __VA_ARGS__); } while (0)

namespace sage {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }       // (null passes: nullable arguments)
inline bool multiples_of(int n, int64_t a, int64_t b, int64_t c = 0) { return a % n == 0 && b % n == 0 && c % n == 0; }
// 16-byte aligned, strides in multiples of n elements
inline bool aligned16_strides(const void *p, int n, int64_t a, int64_t b, int64_t c = 0) { return aligned16(p) && multiples_of(n, a, b, c); }
// the attention kernels form a lane's byte offset into a 64-key tile of int8 k in 32 bits: `row * (int)k_sl + chunk * 16` with row <= 63 and
// chunk * 16 <= D - 16 (sage_attn_body.h, koff), and a clamp of up to 63 rows `* (int)k_sl` (sage_attn_loop_f8.h, the ragged last tile).  Both are
// exact while the largest of them, 63 k_sl + D - 16, is an int -- which also keeps the 1-KiB bias of the ragged tile inside the unsigned offset
inline bool k_tile_fits_int(int64_t k_sl, int D) { return k_sl >= 0 && k_sl < ((int64_t)1 << 31) && 63 * k_sl + D - 16 < ((int64_t)1 << 31); }

}  // namespace sage
