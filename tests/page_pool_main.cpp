// page_pool_main.cpp -- a stand-alone host program over sageattention_amd/csrc/sage_page_pool.h, the arithmetic of the paged KV cache's page pool
// (include/sage_kvpool_gfx950.h): the functions the kernels of sage_kv_pool.hip run on the device.  Built as host code under AddressSanitizer and
// UBSan and run by tests/test_kv_pool_host.py.  Two walks:
//   well-formed programs  random reserve (both forms) / release / fork_prepare steps, with the append's and the fork's effect on the lengths and
//                         the table applied in between.  After every operation
//                           (i)   refcount[p] is the number of (b, e < n_owned[b]) with block_table[b][e] == p,
//                           (ii)  the pages with count 0 are exactly the stack's n_free words, each once,
//                         and after releasing every slot n_free == num_pages.
//   hostile words         the same operations over a workspace, a table, lengths, row counts, prefix words and slot lists filled from a grid of
//                         hostile words -- n_free negative or past num_pages, stack words and table ids outside the pool, n_owned negative or
//                         past the table, a workspace init never wrote.  Every array is allocated at exactly its size, so the sanitizer sees an
//                         index that leaves it, and after every operation
//                           (iii) every table entry the operation changed is -1 or an id in [0, num_pages), every stack word it changed is an id,
//                                 every new_pages word is -1 or an id, every dst_eff word is -1 or a slot, 0 <= granted[b] <= the rows offered.
// Signed overflow inside the arithmetic itself is reported by UBSan.
#include "sage_page_pool.h"

#include <climits>
#include <cstdio>
#include <vector>

namespace {

using namespace sage;

const int WORDS[] = {INT_MIN, INT_MIN + 1, -(1 << 30), -65536, -129, -2, -1, 0, 1, 2, 3, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257,
                     511, 512, 513, 1000, 65535, 65536, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, INT_MAX - 1, INT_MAX};

unsigned long long g_state = 0x9E3779B97F4A7C15ull;
unsigned rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_state >> 33); }
int word() { return WORDS[rnd() % (sizeof(WORDS) / sizeof(WORDS[0]))]; }

long g_ops = 0, g_refused = 0, g_granted = 0, g_forks = 0, g_freed = 0, g_hostile = 0;

struct Pool {
    int N, B, shift, mp, ps, cap;
    std::vector<int> ws, table, lens;
    Pool(int N_, int B_, int shift_, int mp_) : N(N_), B(B_), shift(shift_), mp(mp_), ps(64 << shift_), cap(mp_ * (64 << shift_)),
                                                 ws((size_t)pool_ws_words(N_, B_)), table((size_t)B_ * mp_, -1), lens((size_t)B_, 0)
    {
        for (size_t i = 0; i < ws.size(); i++) ws[i] = pool_init_word(N, B, (long long)i);
    }
    PoolView v() { return pool_view(ws.data(), N, B); }
    PoolTable t() { return PoolTable{table.data(), mp, mp, shift}; }
};

bool fail(const char *what, long a = 0, long b = 0, long c = 0)
{
    std::printf("FAIL %s (%ld, %ld, %ld) after %ld operations\n", what, a, b, c, g_ops);
    return false;
}

// (i) and (ii)
bool invariants(Pool &p)
{
    const PoolView v = p.v();
    std::vector<int> count((size_t)p.N, 0), on_stack((size_t)p.N, 0);
    for (int b = 0; b < p.B; b++) {
        if (v.owned[b] < 0 || v.owned[b] > p.mp) return fail("n_owned out of range", b, v.owned[b]);
        for (int e = 0; e < p.mp; e++) {
            const int id = p.table[(size_t)b * p.mp + e];
            if (e < v.owned[b]) {
                if (id < 0 || id >= p.N) return fail("an owned entry is no page", b, e, id);
                count[(size_t)id]++;
            } else if (id != -1) return fail("an entry nobody owns is not -1", b, e, id);
        }
    }
    if (v.hdr[0] < 0 || v.hdr[0] > p.N) return fail("n_free out of range", v.hdr[0]);
    for (int i = 0; i < v.hdr[0]; i++) {
        if (v.stack[i] < 0 || v.stack[i] >= p.N) return fail("a stack word is no page", i, v.stack[i]);
        on_stack[(size_t)v.stack[i]]++;
    }
    for (int pg = 0; pg < p.N; pg++) {
        if (count[(size_t)pg] != v.refc[pg]) return fail("refcount is not the number of owned entries", pg, v.refc[pg], count[(size_t)pg]);
        if (on_stack[(size_t)pg] != (count[(size_t)pg] == 0 ? 1 : 0)) return fail("the stack is not the pages with count 0, each once", pg, on_stack[(size_t)pg], count[(size_t)pg]);
    }
    return true;
}

// what the append does to the lengths, and sage_kvfork to the table and the lengths (include/sage_kvfork_gfx950.h)
void advance(Pool &p, const std::vector<int> &granted)
{
    for (int b = 0; b < p.B; b++) {
        const int L = pool_clamp(p.lens[(size_t)b], 0, p.cap);
        p.lens[(size_t)b] = L + (granted[(size_t)b] < p.cap - L ? granted[(size_t)b] : p.cap - L);
    }
}
void apply_fork(Pool &p, const std::vector<int> &src, const std::vector<int> &eff, const std::vector<int> &pages, const std::vector<int> *prefix)
{
    for (size_t i = 0; i < src.size(); i++) {
        const int s = src[i], d = eff[i];
        if (s < 0 || s >= p.B || d < 0 || d >= p.B || s == d) continue;
        int P;
        const int np = pool_fork_pages(p.lens[(size_t)s], prefix ? &(*prefix)[i] : nullptr, p.t(), P);
        for (int e = 0; e < np; e++) p.table[(size_t)d * p.mp + e] = p.table[(size_t)s * p.mp + e];
        if (np < p.mp) p.table[(size_t)d * p.mp + np] = pages[i];
        p.lens[(size_t)d] = P;
    }
}

// one random operation; `hostile`: the arguments come from the grid and (iii) is checked in place of (i) and (ii)
bool step(Pool &p, bool hostile)
{
    g_ops++;
    const std::vector<int> table0 = p.table, ws0 = p.ws;
    const PoolView v = p.v();
    const PoolTable t = p.t();
    const unsigned kind = rnd() % 8;
    if (kind < 4) {
        std::vector<int> granted((size_t)p.B, -7), offered((size_t)p.B, 0);
        if (kind < 2) {
            std::vector<int> n((size_t)p.B);
            const int T = hostile ? (word() & 0x7fffffff) | 1 : 1 + (int)(rnd() % (3 * p.ps));
            for (int b = 0; b < p.B; b++) {
                n[(size_t)b] = hostile ? word() : (rnd() % 3 == 0 ? 0 : (rnd() % 3 == 0 ? 1 : (int)(rnd() % (unsigned)(T + 1))));
                offered[(size_t)b] = pool_rows_dense(n[(size_t)b], T);
            }
            pool_reserve_serial(v, t, p.lens.data(), n.data(), T, nullptr, 0, 0, granted.data());
        } else {
            std::vector<int> cu((size_t)p.B + 1, 0);
            int total, max_new;
            if (hostile) {
                for (int &c : cu) c = word();
                total = word(); max_new = word();
            } else {
                max_new = 1 + (int)(rnd() % (3 * p.ps));
                for (int b = 0; b < p.B; b++) cu[(size_t)b + 1] = cu[(size_t)b] + (rnd() % 3 == 0 ? 0 : (int)(rnd() % (unsigned)(max_new + 1)));
                total = cu[(size_t)p.B] > 0 ? cu[(size_t)p.B] : 1;
            }
            for (int b = 0; b < p.B; b++) offered[(size_t)b] = pool_rows_packed(cu[(size_t)b], cu[(size_t)b + 1], total, max_new);
            pool_reserve_serial(v, t, p.lens.data(), nullptr, 0, cu.data(), total, max_new, granted.data());
        }
        for (int b = 0; b < p.B; b++) {
            if (granted[(size_t)b] != 0 && granted[(size_t)b] != offered[(size_t)b]) return fail("granted is neither 0 nor the rows offered", b, granted[(size_t)b], offered[(size_t)b]);
            if (offered[(size_t)b] < 0) return fail("a negative row count", b, offered[(size_t)b]);
            g_granted += granted[(size_t)b] > 0;
        }
        g_refused += v.hdr[1];
        if (v.hdr[1] < 0 || v.hdr[1] > p.B || v.hdr[2] < 0 || v.hdr[3] < 0) return fail("the header of a reserve", v.hdr[1], v.hdr[2], v.hdr[3]);
        if (!hostile) advance(p, granted);
    } else if (kind < 6) {
        const int n = 1 + (int)(rnd() % (unsigned)(p.B + 2));
        std::vector<int> slots((size_t)n);
        for (int i = 0; i < n; i++) slots[(size_t)i] = hostile ? (rnd() % 2 ? word() : (int)(rnd() % (unsigned)p.B)) : (int)(rnd() % (unsigned)(p.B + 2)) - 1;
        if (!hostile)                                    // distinct slots are the caller's contract
            for (int i = 0; i < n; i++)
                for (int j = 0; j < i; j++)
                    if (slots[(size_t)j] == slots[(size_t)i]) slots[(size_t)i] = -1;
        const int before = pool_n_free(v);
        pool_release_serial(v, t, p.lens.data(), slots.data(), n);
        g_freed += pool_n_free(v) - before;
        for (int i = 0; i < n; i++)
            if (slots[(size_t)i] >= 0 && slots[(size_t)i] < p.B && (v.owned[slots[(size_t)i]] != 0 || p.lens[(size_t)slots[(size_t)i]] != 0)) return fail("a released slot keeps something", slots[(size_t)i]);
    } else {
        const int n = 1 + (int)(rnd() % (unsigned)p.B);
        std::vector<int> src((size_t)n), dst((size_t)n), prefix((size_t)n), pages((size_t)n, -7), eff((size_t)n, -7);
        const bool with_prefix = rnd() % 2 != 0;
        const int one = (int)(rnd() % (unsigned)p.B);
        for (int i = 0; i < n; i++) {
            src[(size_t)i] = hostile && rnd() % 3 == 0 ? word() : (rnd() % 2 ? one : (int)(rnd() % (unsigned)p.B));
            dst[(size_t)i] = hostile && rnd() % 3 == 0 ? word() : (int)(rnd() % (unsigned)p.B);
            prefix[(size_t)i] = hostile ? word() : (int)(rnd() % (unsigned)(p.cap + 2)) & (rnd() % 2 ? ~0 : ~(p.ps - 1));
        }
        if (!hostile)                                    // the contract: destinations distinct and disjoint from the sources; a violation is made a refusal
            for (int i = 0; i < n; i++) {
                for (int j = 0; j < n; j++)
                    if (dst[(size_t)i] == src[(size_t)j] || (j < i && dst[(size_t)j] == dst[(size_t)i])) dst[(size_t)i] = -1;
            }
        pool_fork_prepare_serial(v, t, p.lens.data(), src.data(), dst.data(), with_prefix ? prefix.data() : nullptr, n, pages.data(), eff.data());
        for (int i = 0; i < n; i++) {
            if (pages[(size_t)i] < -1 || pages[(size_t)i] >= p.N) return fail("new_pages is neither -1 nor a page", i, pages[(size_t)i]);
            if (eff[(size_t)i] != -1 && (eff[(size_t)i] != dst[(size_t)i] || eff[(size_t)i] < 0 || eff[(size_t)i] >= p.B)) return fail("dst_eff is neither -1 nor the destination", i, eff[(size_t)i]);
            g_forks += eff[(size_t)i] >= 0;
        }
        g_refused += v.hdr[1];
        if (!hostile) apply_fork(p, src, eff, pages, with_prefix ? &prefix : nullptr);
    }
    if (!hostile) return invariants(p);
    // (iii): what the operation wrote
    g_hostile++;
    for (size_t i = 0; i < p.table.size(); i++)
        if (p.table[i] != table0[i] && (p.table[i] < -1 || p.table[i] >= p.N)) return fail("a table entry written by the pool is no page", (long)i, p.table[i]);
    for (int i = 0; i < p.N; i++)
        if (v.stack[i] != ws0[(size_t)(kPoolHdrWords + i)] && (v.stack[i] < 0 || v.stack[i] >= p.N)) return fail("a pushed word is no page", i, v.stack[i]);
    if (v.hdr[0] < 0 || v.hdr[0] > p.N) return fail("n_free written out of range", v.hdr[0]);
    return true;
}

}  // namespace

int main()
{
    const int GEOM[][4] = {{5, 3, 0, 4}, {20, 6, 0, 8}, {9, 6, 1, 8}, {54, 6, 1, 8}, {1, 1, 0, 1}, {3, 2, 2, 2}, {40, 9, 0, 16}, {7, 1024, 0, 1}};      // N, B, page shift, mp
    for (const auto &g : GEOM) {
        for (int program = 0; program < 60; program++) {
            Pool p(g[0], g[1], g[2], g[3]);
            if (!invariants(p)) return 1;
            for (int k = 0; k < 40; k++)
                if (!step(p, false)) return 1;
            std::vector<int> all((size_t)p.B);
            for (int b = 0; b < p.B; b++) all[(size_t)b] = b;
            for (int b0 = 0; b0 < p.B; b0 += 1024) pool_release_serial(p.v(), p.t(), p.lens.data(), all.data() + b0, p.B - b0 < 1024 ? p.B - b0 : 1024);
            if (!invariants(p) || p.ws[0] != p.N) return fail("n_free after releasing every slot", p.ws[0], p.N), 1;
        }
        for (int program = 0; program < 120; program++) {
            Pool p(g[0], g[1], g[2], g[3]);
            const int mode = program % 4;                // 0: a workspace init never wrote; 1: hostile header and n_owned; 2: hostile stack and counts; 3: a hostile table
            for (int k = 0; k < 30; k++) {
                for (size_t i = 0; i < p.ws.size(); i++) {
                    const bool hdr = i < (size_t)kPoolHdrWords, owned = i >= (size_t)kPoolHdrWords + 2 * (size_t)p.N;
                    if (mode == 0 || (mode == 1 && (hdr || owned) && rnd() % 2) || (mode == 2 && !hdr && !owned && rnd() % 2)) p.ws[i] = word();
                }
                if (mode == 0 || mode == 3)
                    for (int &e : p.table)
                        if (rnd() % 2) e = word();
                for (int &l : p.lens)
                    if (rnd() % 2) l = word();
                if (!step(p, true)) return 1;
            }
        }
    }
    if (g_granted < 1000 || g_refused < 1000 || g_forks < 500 || g_freed < 1000 || g_hostile < 10000) return fail("the walk did not reach enough", g_granted, g_refused, g_forks), 1;
    std::printf("every index inside, every id a page: %ld operations (%ld hostile), %ld grants, %ld refusals, %ld forks, %ld pages freed\n", g_ops, g_hostile, g_granted,
                g_refused, g_forks, g_freed);
    return 0;
}
