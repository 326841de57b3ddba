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

}  // namespace sage
