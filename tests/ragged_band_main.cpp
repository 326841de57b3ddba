// ragged_band_main.cpp -- a stand-alone host program over ragged_band (sageattention_amd/csrc/sage_ragged.h), the filter that sorts the samples of
// a step call (include/sage_kvstep_gfx950.h) between its two launches.  Built as host code under AddressSanitizer and UBSan and run by
// tests/test_kv_step_host.py over the hostile words tests/ragged_clamp_main.cpp sweeps.  For every pair of prefix words, total and maximum:
//   (i)   every band result lies inside [0, total] and within max_rows;
//   (ii)  the bands (0, 32] and (32, max_rows] partition ragged_rows' answer: exactly one yields rows when ragged_rows does, with the same
//         (first, rows), and neither does when it does not;
//   (iii) walking every row the two launches would touch -- the decode launch always, the chunk launch when max_rows > 32, as the entry decides
//         it -- stays inside a real buffer of `total` rows (the sanitizer sees any row outside it) and touches no row twice.
// Signed overflow inside the filter itself is reported by UBSan.
#include "sage_ragged.h"

#include <climits>
#include <cstdio>
#include <vector>

int main()
{
    const int words[] = {INT_MIN, INT_MIN + 1, -(1 << 30), -65536, -129, -128, -2, -1, 0, 1, 2, 31, 32, 33, 34, 63, 64, 65, 127, 128, 129, 255, 256, 257,
                         383, 384, 385, 1000, 65535, 65536, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, INT_MAX - 1, INT_MAX};
    const int totals[] = {INT_MIN, -1, 0, 1, 2, 31, 32, 33, 64, 128, 129, 384, 1000, INT_MAX};
    const int maxima[] = {INT_MIN, -1, 0, 1, 31, 32, 33, 64, 128, 129, 1000, INT_MAX};
    const int DECODE = 32;      // rows one wave's slab holds: the decode band's upper edge
    long cases = 0, rows_walked = 0, decode_hits = 0, chunk_hits = 0;
    for (const int total : totals) {
        // the packed tensor of the case: `total` rows of one counter (none for a total the entry points refuse: nothing may then be touched)
        std::vector<unsigned char> rows(total > 0 && total <= 1000 ? (size_t)total : 0);
        for (const int max_rows : maxima)
            for (const int c0 : words)
                for (const int c1 : words) {
                    int f0 = -7, n0 = -7, fd = -7, nd = -7, fc = -7, nc = -7;
                    sage::ragged_rows(c0, c1, total, max_rows, f0, n0);
                    sage::ragged_band(c0, c1, total, max_rows, 0, DECODE, fd, nd);
                    sage::ragged_band(c0, c1, total, max_rows, DECODE, max_rows, fc, nc);
                    const long t = total < 0 ? 0 : total, m = max_rows < 0 ? 0 : max_rows;
                    // (i)
                    const bool inside = fd >= 0 && nd >= 0 && (long)fd + nd <= t && nd <= m && nd <= DECODE &&
                                        fc >= 0 && nc >= 0 && (long)fc + nc <= t && nc <= m && (nc == 0 || nc > DECODE);
                    // (ii)
                    const bool first_same = fd == f0 && fc == f0;
                    const bool split = n0 > 0 ? ((nd == n0) != (nc == n0)) && (nd == 0 || nc == 0) : (nd == 0 && nc == 0);
                    // the chunk launch is only made when max_rows > 32: no sample may need it otherwise
                    const bool host_rule = max_rows > DECODE || nc == 0;
                    if (!inside || !first_same || !split || !host_rule) {
                        std::printf("FAIL c0=%d c1=%d total=%d max=%d -> rows (%d, %d) decode (%d, %d) chunk (%d, %d)\n", c0, c1, total, max_rows, f0, n0, fd,
                                    nd, fc, nc);
                        return 1;
                    }
                    // (iii)
                    if (!rows.empty()) {
                        for (int i = 0; i < nd; i++) { rows[(size_t)fd + i]++; rows_walked++; }
                        if (max_rows > DECODE)
                            for (int i = 0; i < nc; i++) { rows[(size_t)fc + i]++; rows_walked++; }
                        for (int i = 0; i < n0; i++) {
                            if (rows[(size_t)f0 + i] != 1) {
                                std::printf("FAIL c0=%d c1=%d total=%d max=%d: row %d touched %d times\n", c0, c1, total, max_rows, f0 + i, (int)rows[(size_t)f0 + i]);
                                return 1;
                            }
                            rows[(size_t)f0 + i] = 0;
                        }
                    }
                    decode_hits += nd > 0;
                    chunk_hits += nc > 0;
                    cases++;
                }
    }
    if (decode_hits == 0 || chunk_hits == 0) {
        std::printf("FAIL the sweep reached only one band (%ld decode, %ld chunk)\n", decode_hits, chunk_hits);
        return 1;
    }
    std::printf("ragged_band: %ld cases (%ld decode, %ld chunk), %ld rows walked, all inside, none twice\n", cases, decode_hits, chunk_hits, rows_walked);
    return 0;
}
