// sage_page_pool.h -- the arithmetic of the paged KV cache's page pool (include/sage_kvpool_gfx950.h): a free stack, a reference
// count per page and the number of table entries a slot owns, kept in one caller-owned int32 workspace and moved on the device by the lengths.
// One definition for the kernels (sage_kv_pool.hip, device), for the sage_kvpool_*_host entries and for a host program that walks hostile words
// under the sanitizers (tests/page_pool_main.cpp).  Plain C++ with no include beyond sage_ragged.h.
//
// The workspace: hdr[16] = {n_free, slots or forks the last reserve / fork_prepare refused, the pages that call was short of, refusals since
// init, 0 ...}, free_stack[num_pages] (the top, free_stack[n_free - 1], is handed out next), refcount[num_pages], n_owned[B] (the leading entries
// of block_table[b] that hold a reference).  Every word read from it is clamped before anything is formed from it: a workspace init never wrote
// gives wrong numbers, never an index outside the workspace or the table, and never a table entry outside [0, num_pages).
#pragma once
#include "sage_ragged.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SAGE_POOL_HD __host__ __device__
#else
#define SAGE_POOL_HD
#endif

namespace sage {

constexpr int kPoolHdrWords = 16;
constexpr int kPoolFreed = -2147483647 - 1;      // refcount of a page whose last reference a release has just taken, until that release's compaction pushes it

struct PoolView {                   // the workspace's four arrays
    int *hdr, *stack, *refc, *owned;
    int N, B;                       // num_pages >= 1, B >= 1
};
struct PoolTable {                  // the cache's block table
    int *table;                     // [B, mp], row stride `stride` elements
    long stride;
    int mp, page_shift;             // max_pages_per_seq >= 1; page size = 64 << page_shift keys, mp * page size <= 2^30
};

SAGE_POOL_HD inline long long pool_ws_words(int N, int B) { return kPoolHdrWords + 2ll * (N > 0 ? N : 0) + (B > 0 ? B : 0); }
SAGE_POOL_HD inline PoolView pool_view(int *ws, int N, int B) { return PoolView{ws, ws + kPoolHdrWords, ws + kPoolHdrWords + N, ws + kPoolHdrWords + 2l * N, N, B}; }
SAGE_POOL_HD inline int pool_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
SAGE_POOL_HD inline int pool_sat(long long x) { return x < 0 ? 0 : (x > 0x7fffffff ? 0x7fffffff : (int)x); }
SAGE_POOL_HD inline int pool_n_free(const PoolView &v) { return pool_clamp(v.hdr[0], 0, v.N); }
// the k-th page below the top of a stack of nf words, 0 <= k < nf <= N: an id in [0, N) whatever the word holds
SAGE_POOL_HD inline int pool_pop(const PoolView &v, int nf, int k) { return pool_clamp(v.stack[nf - 1 - k], 0, v.N - 1); }

// ---- init: every page free, page 0 on top ---------------------------------------------------------------------------------------------------
SAGE_POOL_HD inline int pool_init_word(int N, int B, long long i)       // word i of a fresh workspace
{
    if (i == 0) return N;
    if (i < kPoolHdrWords) return 0;
    if (i < kPoolHdrWords + (long long)N) return N - 1 - (int)(i - kPoolHdrWords);
    return 0;
}

// ---- reserve --------------------------------------------------------------------------------------------------------------------------------
// rows slot b is about to receive: the dense append's clamp (append_range, sage_kv_cache.h), or the packed append's through the function it uses
SAGE_POOL_HD inline int pool_rows_dense(int new_len, int T) { return pool_clamp(new_len, 0, T > 0 ? T : 0); }
SAGE_POOL_HD inline int pool_rows_packed(int c0, int c1, int total, int max_new)
{
    int first, rows;
    ragged_rows(c0, c1, total, max_new, first, rows);
    return rows;
}
// the entries slot b owns (`own`), those it must own after n rows (`want`) and the pages it needs: cap = mp * page size <= 2^30, so no sum passes 2^31
SAGE_POOL_HD inline int pool_need(int len, int n, int owned_word, const PoolTable &t, int &own, int &want)
{
    const int ps = 64 << t.page_shift, cap = t.mp * ps;
    const int L = pool_clamp(len, 0, cap);
    const int end = n < cap - L ? L + n : cap;
    own = pool_clamp(owned_word, 0, t.mp);
    want = (end + ps - 1) >> (6 + t.page_shift);
    return n > 0 && want > own ? want - own : 0;
}
// slot b granted: `before` pages were popped by the slots in front of it; its own go into block_table[b][own ..] in ascending entry order
SAGE_POOL_HD inline void pool_take(const PoolView &v, const PoolTable &t, int b, int nf, int before, int own, int want)
{
    int *row = t.table + (long)b * t.stride;
    for (int e = own; e < want; e++) {
        const int pg = pool_pop(v, nf, before + (e - own));
        row[e] = pg;
        v.refc[pg] = 1;
    }
    v.owned[b] = want;
}
// the header after a reserve / fork_prepare that popped `popped` pages of nf, refused `refused` items and was asked for `asked` pages in all
SAGE_POOL_HD inline void pool_close_call(const PoolView &v, int nf, int popped, int refused, long long asked)
{
    const int since = v.hdr[3];
    v.hdr[0] = nf - popped;
    v.hdr[1] = refused;
    v.hdr[2] = refused > 0 && asked > nf ? pool_sat(asked - nf) : 0;
    v.hdr[3] = pool_sat((long long)(since < 0 ? 0 : since) + refused);
}

// what sage_kv_pool.hip's one workgroup computes, serially.  Exactly one of new_lens (with T) and cu (with total, max_new) is non-null.
SAGE_POOL_HD inline void pool_reserve_serial(const PoolView &v, const PoolTable &t, const int *lens, const int *new_lens, int T, const int *cu, int total, int max_new,
                                             int *granted)
{
    const int nf = pool_n_free(v);
    long long asked = 0;
    int popped = 0, refused = 0;
    for (int b = 0; b < v.B; b++) {
        const int n = new_lens != nullptr ? pool_rows_dense(new_lens[b], T) : pool_rows_packed(cu[b], cu[b + 1], total, max_new);
        int own, want;
        const int need = pool_need(lens[b], n, v.owned[b], t, own, want);
        asked += need;
        if (need == 0) { granted[b] = n; continue; }
        if (asked > nf) { granted[b] = 0; refused++; continue; }
        pool_take(v, t, b, nf, (int)asked - need, own, want);       // (every slot with a need in front of a granted one was granted)
        popped = (int)asked;
        granted[b] = n;
    }
    pool_close_call(v, nf, popped, refused, asked);
}

// ---- fork_prepare ---------------------------------------------------------------------------------------------------------------------------
// the prefix P of a fork and the whole pages np it shares: include/sage_kvfork_gfx950.h's statements (prefix: null for the whole parent)
SAGE_POOL_HD inline int pool_fork_pages(int len_s, const int *prefix, const PoolTable &t, int &P)
{
    const int cap = t.mp * (64 << t.page_shift);
    const int L = pool_clamp(len_s, 0, cap);
    P = L;
    if (prefix != nullptr) {
        P = pool_clamp(*prefix, 0, L);
        if (P < L) P &= ~63;
    }
    return P >> (6 + t.page_shift);
}
// fork i as far as it does not depend on the stack: -1 if it is refused whatever the stack holds, else the pages it needs (0 or 1)
SAGE_POOL_HD inline int pool_fork_need(const PoolView &v, const PoolTable &t, const int *lens, int s, int d, const int *prefix, int &np)
{
    np = 0;
    if (s < 0 || s >= v.B || d < 0 || d >= v.B || s == d || v.owned[d] != 0) return -1;
    int P;
    np = pool_fork_pages(lens[s], prefix, t, P);
    return np < t.mp ? 1 : 0;
}
// the references a granted fork adds are the caller's (atomic on the device); the rest of a granted fork that popped `before` pages behind it
SAGE_POOL_HD inline void pool_fork_take(const PoolView &v, const PoolTable &t, int d, int np, int need, int nf, int before, int &new_page)
{
    new_page = -1;
    if (need > 0) {
        new_page = pool_pop(v, nf, before);
        v.refc[new_page] = 1;
    }
    v.owned[d] = np + need;
}

SAGE_POOL_HD inline void pool_fork_prepare_serial(const PoolView &v, const PoolTable &t, const int *lens, const int *src, const int *dst, const int *prefix_lens, int n,
                                                  int *new_pages, int *dst_eff)
{
    const int nf = pool_n_free(v);
    long long asked = 0;
    int popped = 0, refused = 0;
    // (the destinations' n_owned are read before any is written: the device reads them all in front of its first barrier)
    for (int i = 0; i < n; i++) {
        int np;
        dst_eff[i] = pool_fork_need(v, t, lens, src[i], dst[i], prefix_lens != nullptr ? prefix_lens + i : nullptr, np);
        new_pages[i] = np;
    }
    for (int i = 0; i < n; i++) {
        const int need = dst_eff[i], np = new_pages[i], s = src[i], d = dst[i];
        if (need > 0) asked += need;
        if (need < 0 || (need > 0 && asked > nf)) { dst_eff[i] = -1; new_pages[i] = -1; refused++; continue; }
        const int *row = t.table + (long)s * t.stride;
        for (int e = 0; e < np; e++)
            if (row[e] >= 0 && row[e] < v.N) v.refc[row[e]] = (int)((unsigned)v.refc[row[e]] + 1u);     // (wraps as the device's atomicAdd does)
        pool_fork_take(v, t, d, np, need, nf, (int)asked - need, new_pages[i]);
        if (need > 0) popped = (int)asked;
        dst_eff[i] = d;
    }
    pool_close_call(v, nf, popped, refused, asked);
}

// ---- release ----------------------------------------------------------------------------------------------------------------------------------
// one reference less for page `id`; the caller that took the last one marks the page (on the device: atomicSub, then the mark)
SAGE_POOL_HD inline void pool_release_slot_serial(const PoolView &v, const PoolTable &t, int *lens, int b)
{
    if (b < 0 || b >= v.B) return;
    const int own = pool_clamp(v.owned[b], 0, t.mp);
    int *row = t.table + (long)b * t.stride;
    for (int e = 0; e < own; e++) {
        const int id = row[e];
        if (id >= 0 && id < v.N) {
            const int old = v.refc[id];
            v.refc[id] = old == 1 ? kPoolFreed : (int)((unsigned)old - 1u);
        }
        row[e] = -1;
    }
    v.owned[b] = 0;
    lens[b] = 0;
}
// the compaction: the marked pages go on the stack highest id first, so that the lowest is handed out next; more than the stack holds are dropped
SAGE_POOL_HD inline void pool_push_freed_serial(const PoolView &v)
{
    int nf = pool_n_free(v);
    for (int p = v.N - 1; p >= 0; p--)
        if (v.refc[p] == kPoolFreed) {
            v.refc[p] = 0;
            if (nf < v.N) v.stack[nf++] = p;
        }
    v.hdr[0] = nf;
}
SAGE_POOL_HD inline void pool_release_serial(const PoolView &v, const PoolTable &t, int *lens, const int *slots, int n)
{
    for (int i = 0; i < n; i++) pool_release_slot_serial(v, t, lens, slots[i]);
    pool_push_freed_serial(v);
}

}  // namespace sage
