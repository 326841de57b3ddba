// ragged_clamp_main.cpp -- a stand-alone host program over ragged_rows (sageattention_amd/csrc/sage_ragged.h), the one clamp between a
// caller-written prefix array and every address the ragged paged kernels form.  Built as host code under AddressSanitizer and UBSan and run by
// tests/test_kv_varlen_host.py: every pair of prefix words out of a set that holds negative, non-monotone, overflowing and past-`total` values
// gives 0 <= first <= first + rows <= total and 0 <= rows <= max_rows, and walking every row the kernel would touch stays inside a real
// buffer of `total` rows (the sanitizer sees any row outside it; signed overflow in the clamp itself is reported by UBSan).
#include "sage_ragged.h"

#include <climits>
#include <cstdio>
#include <vector>

int main()
{
    const int words[] = {INT_MIN, INT_MIN + 1, -(1 << 30), -65536, -129, -128, -2, -1, 0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384,
                         385, 1000, 65535, 65536, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, INT_MAX - 1, INT_MAX};
    const int totals[] = {INT_MIN, -1, 0, 1, 2, 64, 128, 129, 384, 1000, INT_MAX};
    const int maxima[] = {INT_MIN, -1, 0, 1, 64, 128, 129, 1000, INT_MAX};
    long cases = 0, rows_walked = 0;
    for (const int total : totals) {
        // the packed tensor of the case: `total` rows of one element (none for a total the entry points refuse: nothing may then be touched)
        std::vector<unsigned char> rows(total > 0 && total <= 1000 ? (size_t)total : 0);
        for (const int max_rows : maxima)
            for (const int c0 : words)
                for (const int c1 : words) {
                    int first = -7, n = -7;
                    sage::ragged_rows(c0, c1, total, max_rows, first, n);
                    const long t = total < 0 ? 0 : total, m = max_rows < 0 ? 0 : max_rows;
                    const bool ok = first >= 0 && n >= 0 && (long)first + n <= t && n <= m;
                    // a well-formed pair inside the tensor comes back as it is (up to the maximum)
                    const bool well = c0 >= 0 && c0 <= c1 && c1 <= t;
                    const bool same = !well || (first == c0 && n == (c1 - c0 < m ? c1 - c0 : (int)m));
                    if (!ok || !same) {
                        std::printf("FAIL c0=%d c1=%d total=%d max=%d -> first=%d rows=%d\n", c0, c1, total, max_rows, first, n);
                        return 1;
                    }
                    if (!rows.empty() || n == 0)
                        for (int i = 0; i < n && !rows.empty(); i++) { rows[(size_t)first + i]++; rows_walked++; }
                    cases++;
                }
    }
    std::printf("ragged_rows: %ld cases, %ld rows walked, all inside\n", cases, rows_walked);
    return 0;
}
