// step_split_main.cpp -- a stand-alone host program over sageattention_amd/csrc/sage_step_list.h, the arithmetic of the SPLIT step call
// (include/sage_kvlsplit_gfx950.h): which (decode-list rank, chunk, kv head, block) a workgroup of pass 2 takes, which workspace
// rows the three launches form, which table entries a chunk may read.  Built as host code under AddressSanitizer and UBSan and run by
// tests/test_kv_list_split_host.py.  Well-formed and hostile words: S from 2 to 255, groups of 2 to 8 heads, prefix words from
// tests/step_list_main.cpp's grid, list counts and list words of any value.  It proves:
//   (i)   over the grid step_split_grid() sizes, every (r, c, hk, block) with r < the clamped list count is dealt exactly once and nothing else is;
//         the blocks of a unit share an XCD (bid & 7);
//   (ii)  every workspace row index formed -- by pass 1, by pass 2's seed read and partial stores, by the merge -- for whatever the prefix words,
//         the list words and max_seqlen_q hold lies inside a buffer of exactly the bytes the workspace has (the sanitizer sees anything else);
//   (iii) a chunk's table entries lie in [c T, min((c + 1) T, ceil(len / 64))) and nowhere else, the chunks of a sequence partition
//         [0, ceil(len / 64)), and every entry lies inside the sample's row of the table.
// Signed overflow inside the arithmetic itself is reported by UBSan.
#include "sage_step_list.h"

#include <climits>
#include <cstdio>
#include <vector>

namespace {

const int WORDS[] = {INT_MIN, INT_MIN + 1, -(1 << 30), -65536, -129, -128, -2, -1, 0, 1, 2, 31, 32, 33, 34, 63, 64, 65, 127, 128, 129, 255, 256, 257,
                     383, 384, 385, 1000, 65535, 65536, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, INT_MAX - 1, INT_MAX};
const int TOTALS[] = {1, 2, 31, 32, 33, 64, 128, 129, 384, 1000};
const int MAXIMA[] = {1, 5, 31, 32, 33, 64, 128, 129, 1000, INT_MAX};
const int CAPACITIES[] = {64, 128, 1088, 1152, 2560, 65536};

unsigned long long g_state = 0x9E3779B97F4A7C15ull;
unsigned rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_state >> 33); }
template <int N> int pick(const int (&a)[N]) { return a[rnd() % N]; }

long g_grids = 0, g_items = 0, g_rows = 0, g_tiles = 0, g_empty = 0;

inline long long r128(long long x) { return (x + 127) / 128 * 128; }

// (i): the dealing rule over one grid
bool check_grid(int B, int S, int Hkv, int group, int nd_raw)
{
    g_grids++;
    const int nd = nd_raw < 0 ? 0 : (nd_raw < B ? nd_raw : B);          // the kernel's clamp of the list's count
    const int ngb = (group + 3) / 4;
    const long long grid = sage::step_split_grid(B, S, Hkv, group);
    if (grid != 8 * (((long long)B * S * Hkv + 7) / 8) * ngb) { std::printf("FAIL grid\n"); return false; }
    std::vector<int> taken((size_t)nd * S * Hkv * ngb, -1);
    for (long long bid = 0; bid < grid; bid++) {
        int r = -7, c = -7, hk = -7, gb = -7;
        if (!sage::step_split_item((int)bid, nd, S, Hkv, group, r, c, hk, gb)) continue;
        if (r < 0 || r >= nd || c < 0 || c >= S || hk < 0 || hk >= Hkv || gb < 0 || gb >= ngb) {
            std::printf("FAIL item (%d, %d, %d, %d) of bid %lld outside (B=%d S=%d Hkv=%d group=%d nd=%d)\n", r, c, hk, gb, bid, B, S, Hkv, group, nd);
            return false;
        }
        const size_t unit = ((size_t)r * S + c) * Hkv + hk, at = unit * ngb + gb;
        if (taken[at] >= 0) { std::printf("FAIL item (%d, %d, %d, %d) dealt twice\n", r, c, hk, gb); return false; }
        taken[at] = (int)(bid & 7);
        if (taken[unit * ngb] >= 0 && taken[unit * ngb] != (int)(bid & 7)) { std::printf("FAIL the blocks of a unit on two XCDs\n"); return false; }
        g_items++;
    }
    for (const int t : taken)
        if (t < 0) { std::printf("FAIL an item was not dealt (B=%d S=%d Hkv=%d group=%d nd=%d)\n", B, S, Hkv, group, nd); return false; }
    // a workgroup outside the grid's range takes nothing either
    int r, c, hk, gb;
    if (sage::step_split_item(-1, nd, S, Hkv, group, r, c, hk, gb) || sage::step_split_item((int)grid + 8 * ngb, nd, S, Hkv, group, r, c, hk, gb)) {
        std::printf("FAIL a workgroup outside the grid took an item\n");
        return false;
    }
    return true;
}

// (ii): the rows the launches form for one step, into buffers of exactly the workspace's size
bool check_rows(const std::vector<int> &cu, const std::vector<int> &list, int B, int Hkv, int group, int S, int total, int max_q, int D)
{
    const int lq_ws = sage::step_split_ws_rows(max_q);
    if (lq_ws < 1 || lq_ws > 32) { std::printf("FAIL lq_ws %d\n", lq_ws); return false; }
    const long long rows = (long long)B * Hkv * group * S * lq_ws;
    // the layout of _cabi.kv_split_ws_bytes(B, Hq, Lq_ws, D, S): three segments, each rounded up to 128 bytes
    const long long seg = r128(4 * rows), bytes = 2 * seg + r128(4 * rows * D);
    std::vector<float> chunk_max((size_t)rows), lse_part((size_t)rows);      // (exact sizes: the sanitizer's)
    std::vector<char> o_rows((size_t)rows, 0);
    if (bytes < 4 * rows * (2 + (long long)D)) { std::printf("FAIL ws bytes\n"); return false; }
    for (int b = 0; b < B; b++) {
        int first, n;
        sage::ragged_band(cu[b], cu[b + 1], total, max_q, 0, sage::kStepDecodeRows, first, n);
        if (n < 0 || n > lq_ws || first < 0 || (long long)first + n > total) { std::printf("FAIL band rows %d (lq_ws %d) first %d total %d\n", n, lq_ws, first, total); return false; }
        for (int hk = 0; hk < Hkv; hk++)
            for (int c = 0; c < S; c += (S > 16 ? 1 + (int)(rnd() % 7) : 1))
                for (int gq = 0; gq < group; gq++)
                    for (int l = 0; l < n; l++) {
                        const long long r = sage::step_split_ws_row(b, hk, c, gq, l, Hkv, S, group, lq_ws);
                        if (r < 0 || r >= rows) { std::printf("FAIL ws row %lld of %lld\n", r, rows); return false; }
                        chunk_max[(size_t)r] = 1.0f;                   // pass 1's store, pass 2's seed read
                        lse_part[(size_t)r] = 1.0f;                    // pass 2's LSE store, the merge's read
                        o_rows[(size_t)r]++;                           // pass 2's partial row (D floats at r * D), the merge's read
                        g_rows++;
                    }
    }
    // pass 2 through the list: any word, clamped as the kernel clamps it, names a sequence whose rows lie inside as well
    const int nd_raw = list[0];
    const int nd = nd_raw < 0 ? 0 : (nd_raw < B ? nd_raw : B);
    const long long grid = sage::step_split_grid(B, S, Hkv, group);
    for (long long bid = 0; bid < grid; bid += 1 + (long long)(rnd() % 5)) {
        int r, c, hk0, gb;
        if (!sage::step_split_item((int)bid, nd, S, Hkv, group, r, c, hk0, gb)) continue;
        const int bl = list[1 + r], b = bl < 0 ? 0 : (bl < B ? bl : B - 1);
        int first, n;
        sage::ragged_band(cu[b], cu[b + 1], total, max_q, 0, sage::kStepDecodeRows, first, n);
        for (int w = 0; w < 4; w++) {
            const int hw = 4 * gb + w;
            if (hw >= group) continue;
            // the body's indices: lse_part[(b * Hq' + h) * lq_ws + row] with Hq' = Hkv * S * group, h = (hk0 * S + c) * group + hw; the seed row of chunk c' <= c
            for (int l = 0; l < n; l++) {
                const long long h = ((long long)hk0 * S + c) * group + hw;
                const long long li = ((long long)b * Hkv * S * group + h) * lq_ws + l;
                const long long si = ((long long)b * Hkv + hk0) * S * ((long long)group * lq_ws) + (long long)hw * lq_ws + l + (long long)c * group * lq_ws;
                if (li != sage::step_split_ws_row(b, hk0, c, hw, l, Hkv, S, group, lq_ws) || si != li) { std::printf("FAIL the body's index is not the layout's\n"); return false; }
                lse_part[(size_t)li] = 2.0f;
                chunk_max[(size_t)si] = 2.0f;
            }
        }
    }
    return true;
}

// (iii): the tiles of the chunks of one sequence
bool check_tiles(int Lk, int S, int len_raw)
{
    const int T = sage::step_split_tiles(Lk, S);
    const int len = len_raw < 0 ? 0 : (len_raw < Lk ? len_raw : Lk);
    const int nt = (len + 63) / 64, cap_tiles = (Lk + 63) / 64;
    if (T < 1 || (long long)T * S < cap_tiles || (long long)(T - 1) * S >= cap_tiles + S) { std::printf("FAIL T %d (Lk %d, S %d)\n", T, Lk, S); return false; }
    std::vector<char> seen((size_t)cap_tiles, 0);              // the sample's row of the table, one entry per tile here: exactly its size
    for (int c = 0; c < S; c++) {
        int t0, t1;
        sage::step_split_tile_range(c, T, len, t0, t1);
        if (t0 != c * T || t1 < t0) { std::printf("FAIL range c %d: [%d, %d)\n", c, t0, t1); return false; }
        const long long e = (long long)(c + 1) * T < nt ? (long long)(c + 1) * T : nt;
        if (t1 != (e > t0 ? e : t0)) { std::printf("FAIL range end c %d: %d, want %lld\n", c, t1, e); return false; }
        g_empty += t1 == t0;
        for (int t = t0; t < t1; t++) {
            if (seen[(size_t)t]) { std::printf("FAIL tile %d read by two chunks\n", t); return false; }
            seen[(size_t)t] = 1;
            g_tiles++;
        }
    }
    for (int t = 0; t < cap_tiles; t++)
        if ((seen[(size_t)t] != 0) != (t < nt)) { std::printf("FAIL tile %d of %d (len %d): read %d\n", t, nt, len, seen[(size_t)t]); return false; }
    return true;
}

}  // namespace

int main()
{
    // (i) every S, every group, B and Hkv around the octet's edges, list counts of any value
    const int counts[] = {INT_MIN, -1, 0, 1, 2, 3, 5, 8, 9, 1024, INT_MAX};
    for (int S = 2; S <= 255; S++)
        for (int group = 2; group <= 8; group++)
            for (const int B : {1, 2, 3, 5, 9})
                for (const int Hkv : {1, 2, 3, 8})
                    if ((S < 20 || S > 250 || (S + group + B + Hkv) % 7 == 0) && !check_grid(B, S, Hkv, group, pick(counts))) return 1;
    for (int S = 2; S <= 255; S++)
        for (int group = 2; group <= 8; group++)
            if (!check_grid(4, S, 2, group, 4) || !check_grid(1, S, 1, group, 1)) return 1;
    // (ii) hostile and well-formed prefix words, list words of any value
    for (int n = 0; n < 6000; n++) {
        const int B = 1 + (int)(rnd() % 9), Hkv = 1 + (int)(rnd() % 3), group = 2 + (int)(rnd() % 7), S = 2 + (int)(rnd() % 254);
        const int total = pick(TOTALS), max_q = pick(MAXIMA);
        std::vector<int> cu(B + 1), list(B + 1);
        if (n % 3 == 0) { for (int &w : cu) w = pick(WORDS); }
        else if (n % 3 == 1) { for (int &w : cu) w = (int)(rnd() % (unsigned)(total + 40)); }
        else { cu[0] = 0; for (int b = 0; b < B; b++) { const int c[] = {0, 1, 1, 2, 5, 31, 32, 33, 40, 130}; cu[b + 1] = cu[b] + pick(c); } }
        for (int &w : list) w = (n & 1) ? pick(WORDS) : (int)(rnd() % (unsigned)(B + 2));
        if (!check_rows(cu, list, B, Hkv, group, S, total, max_q, (n & 2) ? 64 : 128)) return 1;
    }
    // (iii) every S over the capacities, lengths around every chunk's edges and hostile ones
    for (const int Lk : CAPACITIES)
        for (int S = 2; S <= 255; S++) {
            const int T = sage::step_split_tiles(Lk, S);
            for (const int len : WORDS)
                if (!check_tiles(Lk, S, len)) return 1;
            for (int c = 0; c <= S; c += (S > 24 ? 1 + (int)(rnd() % 9) : 1))
                for (const int d : {-65, -64, -63, -1, 0, 1, 63, 64, 65})
                    if (!check_tiles(Lk, S, (int)((long long)c * T * 64 + d))) return 1;
        }
    if (g_items == 0 || g_rows == 0 || g_tiles == 0 || g_empty == 0) { std::printf("FAIL the sweep missed a part\n"); return 1; }
    std::printf("step_split: %ld grids, %ld items each dealt once, %ld workspace rows, %ld tiles each in its own chunk (%ld chunks empty), all inside, none twice\n", g_grids, g_items,
                g_rows, g_tiles, g_empty);
    return 0;
}
