// step_list_main.cpp -- a stand-alone host program over sageattention_amd/csrc/sage_step_list.h, the arithmetic of the listed step call's two work
// lists (include/sage_kvlist_gfx950.h): the functions the plan kernel runs on the device.  Built as host code under AddressSanitizer and UBSan and
// run by tests/test_kv_list_host.py.  The inputs are hostile prefix, length and offset words -- the grid tests/ragged_band_main.cpp sweeps,
// extended by kv_lens, q_start and the window -- for B = 1 over the whole grid and for B = 2 .. 9 drawn from it, plus well-formed steps.  For
// every case:
//   (i)   the ranks of each list are a permutation of [0, n): every rank is taken exactly once;
//   (ii)  weights never increase along a list;
//   (iii) every written entry names a sequence of the list's class -- and, in the chunk list, a block that sequence has;
//   (iv)  a well-formed prefix array never exceeds the host-known bound (no work is dropped);
//   (v)   any other is clamped: the workspace is allocated at exactly its size, so the sanitizer sees a write at or past the cap, and the entries
//         past the two counts keep their fill.
// Signed overflow inside the arithmetic itself is reported by UBSan.
#include "sage_step_list.h"

#include <climits>
#include <cstdio>
#include <vector>

namespace {

const int WORDS[] = {INT_MIN, INT_MIN + 1, -(1 << 30), -65536, -129, -128, -2, -1, 0, 1, 2, 31, 32, 33, 34, 63, 64, 65, 127, 128, 129, 255, 256, 257,
                     383, 384, 385, 1000, 65535, 65536, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, INT_MAX - 1, INT_MAX};
const int TOTALS[] = {INT_MIN, -1, 0, 1, 2, 31, 32, 33, 64, 128, 129, 384, 1000, INT_MAX};
const int MAXIMA[] = {INT_MIN, -1, 0, 1, 31, 32, 33, 64, 128, 129, 1000, INT_MAX};
const int WINDOWS[] = {0, 0, 1, 63, 64, 200, 1 << 30, INT_MAX};
const int CAPACITIES[] = {64, 1024, 65536, 1 << 30};
const int FILL = -77;

unsigned long long g_state = 0x9E3779B97F4A7C15ull;
unsigned rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_state >> 33); }
template <int N> int pick(const int (&a)[N]) { return a[rnd() % N]; }

long g_cases = 0, g_listed = 0, g_decode = 0, g_chunk = 0, g_clamped = 0, g_wellformed = 0, g_windowed = 0;

// one step: false (after a message) if any of (i) .. (v) fails
bool check(const std::vector<int> &cu, const std::vector<int> &kv, const std::vector<int> &qs, int B, int total, int max_q, int Lk, int window, bool well_formed)
{
    g_cases++;
    const int cap = sage::step_weight_cap(window);
    std::vector<sage::StepSeq> seq(B);
    std::vector<int> rows(B), lk(B), dw(B);
    long long n_all = 0;
    int n_decode = 0;
    const long long t = total < 0 ? 0 : total, m = max_q < 0 ? 0 : max_q;
    for (int b = 0; b < B; b++) {
        const sage::StepSeq s = seq[b] = sage::step_seq(cu[b], cu[b + 1], total, max_q, kv[b], qs[b], Lk, window);
        const bool cls_ok = s.cls == sage::STEP_IDLE ? s.rows == 0 : s.cls == sage::STEP_DECODE ? (s.rows >= 1 && s.rows <= 32) : (s.cls == sage::STEP_CHUNK && s.rows > 32);
        if (!cls_ok || s.first < 0 || s.rows < 0 || (long long)s.first + s.rows > t || s.rows > m || s.len < 0 || s.len > Lk || s.lk_eff < 0 || s.lk_eff > s.len) {
            std::printf("FAIL step_seq b=%d words (%d, %d) total=%d max=%d kv=%d qs=%d Lk=%d W=%d -> cls %d first %d rows %d len %d lk_eff %d\n", b, cu[b], cu[b + 1], total,
                        max_q, kv[b], qs[b], Lk, window, s.cls, s.first, s.rows, s.len, s.lk_eff);
            return false;
        }
        rows[b] = s.cls == sage::STEP_CHUNK ? s.rows : 0;
        lk[b] = s.lk_eff;
        dw[b] = s.cls == sage::STEP_DECODE ? sage::step_decode_weight(s.lk_eff, cap) : -1;
        n_decode += s.cls == sage::STEP_DECODE;
        n_all += sage::step_blocks(rows[b]);
        // the first, the middle and the last block's weights: inside [0, cap], not decreasing with the block
        const int nq = sage::step_blocks(rows[b]);
        if (nq > 0) {
            const int w0 = sage::step_chunk_weight(rows[b], lk[b], 0, cap), w1 = sage::step_chunk_weight(rows[b], lk[b], nq / 2, cap),
                      w2 = sage::step_chunk_weight(rows[b], lk[b], nq - 1, cap);
            if (w0 < 0 || w0 > w1 || w1 > w2 || w2 > cap) { std::printf("FAIL weights b=%d rows=%d lk=%d: %d %d %d cap %d\n", b, rows[b], lk[b], w0, w1, w2, cap); return false; }
        }
    }
    const long long bound = sage::step_chunk_bound(B, total, max_q);
    if (bound < 0) { std::printf("FAIL bound %lld\n", bound); return false; }
    // (iv): max_seqlen_q <= 32 makes no chunk launch and admits no chunk sequence
    if (well_formed && n_all > bound) { std::printf("FAIL well-formed step of %lld chunk items, bound %lld (B=%d total=%d max=%d)\n", n_all, bound, B, total, max_q); return false; }
    if (max_q <= 32 && n_all != 0) { std::printf("FAIL a chunk sequence under max_seqlen_q = %d\n", max_q); return false; }
    if (n_all > 20000 || bound > 20000) return true;          // (the words' own extremes: a list no entry point admits -- the per-sequence checks above stand)
    g_listed++;
    g_wellformed += well_formed;
    g_windowed += window > 0;
    // (i) by the rank functions themselves
    std::vector<char> seen((size_t)n_all, 0);
    for (int b = 0; b < B; b++)
        for (int j = 0; j < sage::step_blocks(rows[b]); j++) {
            const int r = sage::step_chunk_rank(rows.data(), lk.data(), B, b, j, cap);
            if (r < 0 || r >= n_all || seen[(size_t)r]) { std::printf("FAIL chunk rank %d of (%d, %d), %lld items (taken twice or outside)\n", r, b, j, n_all); return false; }
            seen[(size_t)r] = 1;
        }
    std::vector<char> seen_d((size_t)B, 0);
    for (int b = 0; b < B; b++)
        if (dw[b] >= 0) {
            const int r = sage::step_decode_rank(dw.data(), B, b);
            if (r < 0 || r >= n_decode || seen_d[(size_t)r]) { std::printf("FAIL decode rank %d of %d, %d sequences\n", r, b, n_decode); return false; }
            seen_d[(size_t)r] = 1;
        }
    // the plan as the device writes it, into a workspace of exactly its size: (v) is the sanitizer's
    const size_t words = (size_t)sage::step_ws_words(B, total, max_q);
    if (words != (size_t)sage::kStepHdrWords + (size_t)B + 2 * (size_t)bound) { std::printf("FAIL ws words\n"); return false; }
    int *const ws = new int[words];
    for (size_t i = 0; i < words; i++) ws[i] = FILL;
    std::vector<int> s0(B), s1(B), s2(B);
    sage::step_plan_serial(cu.data(), kv.data(), qs.data(), B, total, max_q, Lk, window, 8, 2, 128, (int)bound, s0.data(), s1.data(), s2.data(), ws);
    bool ok = true;
    const int nd = ws[0], nc = ws[1];
    const int *const dl = ws + sage::kStepHdrWords, *const items = dl + B;
    if (nd != n_decode || nc != (n_all < bound ? n_all : bound) || ws[5] != n_all || ws[2] < 1 || (ws[3] != 0 && ws[3] != 1) || ws[4] != 0) ok = false;
    g_clamped += n_all > bound;
    for (int r = 0; ok && r < B; r++) {
        if (r >= nd) { ok = dl[r] == FILL; continue; }
        const int b = dl[r];
        ok = b >= 0 && b < B && seq[b].cls == sage::STEP_DECODE && (r == 0 || dw[dl[r - 1]] >= dw[b]);      // (ii), (iii)
    }
    for (long long r = 0; ok && r < bound; r++) {
        const int b = items[2 * r], j = items[2 * r + 1];
        if (r >= nc) { ok = b == FILL && j == FILL; continue; }
        ok = b >= 0 && b < B && seq[b].cls == sage::STEP_CHUNK && j >= 0 && j < sage::step_blocks(rows[b]);      // (iii)
        if (ok && r > 0) {
            const int pb = items[2 * r - 2], pj = items[2 * r - 1];
            const int wp = sage::step_chunk_weight(rows[pb], lk[pb], pj, cap), w = sage::step_chunk_weight(rows[b], lk[b], j, cap);
            ok = wp > w || (wp == w && (pb < b || (pb == b && pj > j)));       // (ii), and the order's two tie-breaks
        }
    }
    if (!ok) {
        std::printf("FAIL plan B=%d total=%d max=%d Lk=%d W=%d: n_decode %d (%d), n_chunk %d of %lld, bound %lld\n", B, total, max_q, Lk, window, nd, n_decode, nc, n_all, bound);
        for (int b = 0; b <= B; b++) std::printf("  cu[%d] = %d\n", b, cu[b]);
    }
    g_decode += nd;
    g_chunk += nc;
    delete[] ws;
    return ok;
}

}  // namespace

int main()
{
    // B = 1: the whole grid of ragged_band_main.cpp, each case with three draws of (kv_lens, q_start, window, capacity)
    for (const int total : TOTALS)
        for (const int max_q : MAXIMA)
            for (const int c0 : WORDS)
                for (const int c1 : WORDS)
                    for (int d = 0; d < 3; d++)
                        if (!check({c0, c1}, {pick(WORDS)}, {pick(WORDS)}, 1, total, max_q, pick(CAPACITIES), pick(WINDOWS), false)) return 1;
    // B = 2 .. 9: hostile words drawn from the grid
    for (int B = 2; B <= 9; B++)
        for (int n = 0; n < 40000; n++) {
            std::vector<int> cu(B + 1), kv(B), qs(B);
            for (int &w : cu) w = pick(WORDS);
            // (half of the cases: small non-monotone words, so that several sequences overlap inside the tensor and the cap is reached)
            if (n & 1) for (int &w : cu) w = (int)(rnd() % 1001);
            for (int &w : kv) w = pick(WORDS);
            for (int &w : qs) w = pick(WORDS);
            if (!check(cu, kv, qs, B, pick(TOTALS), pick(MAXIMA), pick(CAPACITIES), pick(WINDOWS), false)) return 1;
        }
    // B = 1 .. 9: well-formed steps -- counts around the class and block edges, contexts and offsets as a serving engine has them or hostile
    const int counts[] = {0, 0, 1, 1, 2, 31, 32, 33, 40, 127, 128, 129, 130, 256, 257, 260, 385};
    for (int B = 1; B <= 9; B++)
        for (int n = 0; n < 40000; n++) {
            std::vector<int> cu(B + 1), kv(B), qs(B);
            cu[0] = (int)(rnd() % 3);
            int most = 1;
            for (int b = 0; b < B; b++) {
                const int c = pick(counts);
                cu[b + 1] = cu[b] + c;
                most = c > most ? c : most;
                kv[b] = (n & 2) ? pick(WORDS) : (int)(rnd() % 1100);
                const long long br = (long long)kv[b] - c;      // (bottom-right, as the Python layer forms it: clamped into an int)
                qs[b] = (n & 4) ? pick(WORDS) : (int)(br < INT_MIN ? INT_MIN : br);
            }
            const int total = cu[B] + (int)(rnd() % 3), max_q = (n & 8) ? most : pick(MAXIMA);
            if (total < 1) continue;
            if (!check(cu, kv, qs, B, total, max_q, 1024, pick(WINDOWS), true)) return 1;
        }
    if (g_decode == 0 || g_chunk == 0 || g_clamped == 0 || g_wellformed == 0 || g_windowed == 0) {
        std::printf("FAIL the sweep missed a part (%ld decode entries, %ld chunk entries, %ld clamped, %ld well-formed, %ld windowed)\n", g_decode, g_chunk, g_clamped,
                    g_wellformed, g_windowed);
        return 1;
    }
    std::printf("step_list: %ld cases, %ld listed (%ld well-formed, %ld clamped to the cap, %ld under a window), %ld decode and %ld chunk entries, "
                "every rank once, weights in order, all inside\n", g_cases, g_listed, g_wellformed, g_clamped, g_windowed, g_decode, g_chunk);
    return 0;
}
