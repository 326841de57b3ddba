// sage_step_list.h -- the arithmetic of the LISTED step call's two work lists (include/sage_kvlist_gfx950.h): which class a
// sequence of a step falls into, what its items weigh, where each item stands in its list and how many a list can hold.  One definition for the
// plan kernel (sage_kv_list_plan.hip, device), for sage_kvlist_plan_host and for a host program that walks hostile words under the sanitizers
// (tests/step_list_main.cpp).  Plain C++ with no include beyond sage_ragged.h and sage_work_order.h.
//
// The lists only ORDER work: the kernels read the prefix words again and decide by ragged_band themselves, so a wrong list gives wrong
// scheduling -- or, malformed input, dropped work -- and never another result for a row that is computed.
#pragma once
#include "sage_ragged.h"
#include "sage_work_order.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SAGE_STEP_HD __host__ __device__
#else
#define SAGE_STEP_HD
#endif

namespace sage {

enum : int { STEP_IDLE = 0, STEP_DECODE = 1, STEP_CHUNK = 2 };
constexpr int kStepDecodeRows = 32;      // the decode band is (0, 32], the chunk band (32, max_seqlen_q]: the step call's two BandArgs
constexpr int kStepHdrWords = 16;        // hdr: n_decode, n_chunk_items, group, fold, left, chunk items before the clamp, max key count of a chunk sequence, 0 ...

struct StepSeq {
    int cls;        // STEP_*
    int first;      // the sequence's first packed row (ragged_rows' clamp)
    int rows;       // n_b: the clamped row count if the sequence lies in a band, else 0
    int len;        // len_b: the key count, clamped to [0, Lk] as the body clamps it
    int lk_eff;     // clamp(qstart_b + n_b, 0, len_b): the keys up to the last row's diagonal
};

// ceil(rows / 128) for rows in [0, INT_MAX]: no sum is formed
SAGE_STEP_HD inline int step_blocks(int rows) { return (rows >> 7) + ((rows & 127) != 0 ? 1 : 0); }

// the cap of an item's weight under a window of W keys: a block of 128 rows then visits at most ceil((W + 128) / 64) + 1 tiles
SAGE_STEP_HD inline int step_weight_cap(int window)
{
    if (window <= 0) return 0x7fffffff;
    const int w = window < (1 << 30) ? window : (1 << 30);
    return ((w + 128 + 63) >> 6) + 1;
}

// Sequence b of a step from its words.  The row count and the class come from ragged_band itself -- the two bands the step call's launches
// carry -- so there is no second statement of the clamp; len_b and qstart_b are clamped as the kernel body clamps them (the KVLEN / QSTART /
// WINDOW statements of the dense branch, with the sample's own row count: RAGGED).  Sums are formed in 64 bits: whatever the words hold.
SAGE_STEP_HD inline StepSeq step_seq(int c0, int c1, int total_q, int max_seqlen_q, int kv_len, int q_start, int Lk, int window)
{
    StepSeq s;
    int nd, nc, first2;
    ragged_band(c0, c1, total_q, max_seqlen_q, 0, kStepDecodeRows, s.first, nd);
    ragged_band(c0, c1, total_q, max_seqlen_q, kStepDecodeRows, max_seqlen_q, first2, nc);
    s.rows = nd > 0 ? nd : nc;
    s.cls = nd > 0 ? STEP_DECODE : (nc > 0 ? STEP_CHUNK : STEP_IDLE);
    const int n = s.rows, cap = Lk > 0 ? Lk : 0;
    s.len = kv_len < 0 ? 0 : (kv_len < cap ? kv_len : cap);
    long long qs;
    if (window > 0) {
        const int wwin = window < (1 << 30) ? window : (1 << 30);
        const int sl = q_start < -n ? -n : q_start;
        qs = (long long)sl - cap > wwin ? (long long)cap + wwin : sl;
    } else
        qs = q_start < -n ? -n : (q_start < cap ? q_start : cap);
    const long long e = qs + n;
    s.lk_eff = e < 0 ? 0 : (e < s.len ? (int)e : s.len);
    return s;
}

// ---- chunk items: (sequence, 128-row query block) -----------------------------------------------------------------------------------------
// weight: the 64-key tiles block j visits under the bottom-right mask of a sequence of n rows whose last row's diagonal stands at key
// lk_eff - 1, capped under a window.  It orders the list only.
SAGE_STEP_HD inline int step_chunk_weight(int n, int lk_eff, int j, int cap)
{
    const int w = varlen_item_weight(n, lk_eff, j, 2);
    return w < cap ? w : cap;
}

// number of blocks j in [0, nq) of that sequence whose capped weight is > w: none if w has reached the cap, else those whose own weight is
SAGE_STEP_HD inline int step_chunk_heavier(int nq, int n, int lk_eff, int w, int cap)
{
    return w >= cap ? 0 : varlen_count_heavier(nq, n, lk_eff, w, 2);
}

// rank of item (s, j) in the list sorted by (weight descending, sequence ascending, query block descending) -- varlen_item_rank with the cap.
// rows[t]: the row count of a CHUNK sequence, 0 for every other (no block, no item); lk[t]: its lk_eff.  A total order whatever the words hold.
SAGE_STEP_HD inline int step_chunk_rank(const int *rows, const int *lk, int nseq, int s, int j, int cap)
{
    const int w = step_chunk_weight(rows[s], lk[s], j, cap);
    int rank = 0;
    for (int t = 0; t < nseq; t++) {
        const int nq = step_blocks(rows[t]);
        const int gt = step_chunk_heavier(nq, rows[t], lk[t], w, cap);
        rank += gt;
        if (t < s) rank += step_chunk_heavier(nq, rows[t], lk[t], w - 1, cap) - gt;      // equal weight, earlier sequence
    }
    // equal weight, same sequence, later block: capped weights do not decrease with j either
    const int nq_s = step_blocks(rows[s]);
    rank += (nq_s - step_chunk_heavier(nq_s, rows[s], lk[s], w, cap)) - 1 - j;
    return rank;
}

// ---- decode items: one per sequence -------------------------------------------------------------------------------------------------------
SAGE_STEP_HD inline int step_decode_weight(int lk_eff, int cap)
{
    const int w = (lk_eff + 63) >> 6;
    return w < cap ? w : cap;
}

// rank by (weight descending, sequence ascending), by counting.  dw[t]: the weight of a DECODE sequence, -1 for every other
SAGE_STEP_HD inline int step_decode_rank(const int *dw, int nseq, int s)
{
    int rank = 0;
    for (int t = 0; t < nseq; t++) rank += (dw[t] >= 0 && (dw[t] > dw[s] || (dw[t] == dw[s] && t < s))) ? 1 : 0;
    return rank;
}

// ---- host-known sizes ---------------------------------------------------------------------------------------------------------------------
// chunk items of a well-formed prefix array: a chunk sequence has at least 33 rows, so there are at most min(B, total_q / 33) of them, and
// sum ceil(n_i / 128) <= floor(sum n_i / 128) + their number; never more than the dense grid's B * ceil(max_seqlen_q / 128).  (long long: the
// product may pass 2^31 for arguments no entry point admits)
SAGE_STEP_HD inline long long step_chunk_bound(int B, int total_q, int max_seqlen_q)
{
    if (B <= 0 || total_q <= kStepDecodeRows || max_seqlen_q <= kStepDecodeRows) return 0;
    const long long dense = (long long)B * (((long long)max_seqlen_q + 127) / 128);
    const int nchunk = total_q / (kStepDecodeRows + 1);
    const long long packed = (long long)(total_q / 128) + (B < nchunk ? B : nchunk);
    return dense < packed ? dense : packed;
}
SAGE_STEP_HD inline long long step_ws_words(int B, int total_q, int max_seqlen_q)
{
    return kStepHdrWords + (long long)(B > 0 ? B : 0) + 2 * step_chunk_bound(B, total_q, max_seqlen_q);
}
SAGE_STEP_HD inline long long step_decode_grid(int B, int Hkv, int group) { return 8 * (((long long)B * Hkv + 7) / 8) * ((group + 3) / 4); }
SAGE_STEP_HD inline long long step_chunk_grid(int Hq, long long bound) { return 8 * ((Hq & 7) * ((bound + 7) / 8) + (Hq >> 3) * bound); }

// ---- the plan's header, and the whole plan in one thread ------------------------------------------------------------------------------------
// n_chunk_all: the chunk items the words give; the list holds min(n_chunk_all, items_cap) -- a malformed prefix array drops work, it never
// writes past the cap.  group / fold / left: plan_varlen_order over Hq heads of that many items.
SAGE_STEP_HD inline void step_write_hdr(int *hdr, int n_decode, int n_chunk_all, int items_cap, int max_len, int Hq, int Hkv, int head_dim)
{
    const int cap = items_cap > 0 ? items_cap : 0;
    const int n_chunk = n_chunk_all < cap ? (n_chunk_all > 0 ? n_chunk_all : 0) : cap;
    WorkOrder w;
    plan_varlen_order(w, Hq, Hkv > 0 ? Hq / Hkv : 1, n_chunk, (long)max_len, head_dim, true);
    hdr[0] = n_decode; hdr[1] = n_chunk; hdr[2] = w.group; hdr[3] = w.fold; hdr[4] = w.left;
    hdr[5] = n_chunk_all; hdr[6] = max_len;
    for (int i = 7; i < kStepHdrWords; i++) hdr[i] = 0;
}

// what sage_kv_list_plan.hip's one workgroup computes, serially: ws = hdr[kStepHdrWords], decode_list[B], chunk_items[2 * items_cap].  rows / lk /
// dw: three scratch arrays of B ints.  Entries of the lists past their counts are not written.
SAGE_STEP_HD inline void step_plan_serial(const int *cu_q, const int *kv_lens, const int *q_start, int B, int total_q, int max_seqlen_q, int Lk, int window,
                                          int Hq, int Hkv, int head_dim, int items_cap, int *rows, int *lk, int *dw, int *ws)
{
    const int cap = step_weight_cap(window);
    int n_decode = 0, max_len = 0;
    long long n_all = 0;
    for (int b = 0; b < B; b++) {
        const StepSeq s = step_seq(cu_q[b], cu_q[b + 1], total_q, max_seqlen_q, kv_lens[b], q_start[b], Lk, window);
        rows[b] = s.cls == STEP_CHUNK ? s.rows : 0;
        lk[b] = s.lk_eff;
        dw[b] = s.cls == STEP_DECODE ? step_decode_weight(s.lk_eff, cap) : -1;
        n_decode += s.cls == STEP_DECODE ? 1 : 0;
        if (s.cls == STEP_CHUNK) { n_all += step_blocks(s.rows); max_len = s.len > max_len ? s.len : max_len; }
    }
    const int n_chunk_all = n_all < 0x7fffffff ? (int)n_all : 0x7fffffff;
    step_write_hdr(ws, n_decode, n_chunk_all, items_cap, max_len, Hq, Hkv, head_dim);
    int *const decode_list = ws + kStepHdrWords, *const items = decode_list + B;
    const int n_chunk = ws[1];
    for (int b = 0; b < B; b++) {
        if (dw[b] >= 0) decode_list[step_decode_rank(dw, B, b)] = b;
        for (int j = 0; j < step_blocks(rows[b]); j++) {
            const int rank = step_chunk_rank(rows, lk, B, b, j, cap);
            if (rank >= 0 && rank < n_chunk) { items[2 * rank] = b; items[2 * rank + 1] = j; }
        }
    }
}

// ---- the split step call (include/sage_kvlsplit_gfx950.h): every decode sequence as S key-range chunks ------------------------
// A chunk is T whole 64-key tiles of the LOGICAL key axis (3.20's rule): T = ceil(ceil(Lk / 64) / S), the same for every sequence of the call.
SAGE_STEP_HD inline int step_split_tiles(int Lk, int S)
{
    const long long nt = ((long long)(Lk > 0 ? Lk : 0) + 63) >> 6;
    return S > 0 ? (int)((nt + S - 1) / S) : 0;
}
// the rows per (sequence, head) of the split workspace: what a decode sequence can have under this max_seqlen_q
SAGE_STEP_HD inline int step_split_ws_rows(int max_seqlen_q) { return max_seqlen_q < kStepDecodeRows ? (max_seqlen_q > 0 ? max_seqlen_q : 0) : kStepDecodeRows; }
// pass 2's grid: units (decode-list rank r, chunk c, kv head hk), u = (r * S + c) * Hkv + hk, in whole octets, ceil(group / 4) blocks each
SAGE_STEP_HD inline long long step_split_grid(int B, int S, int Hkv, int group) { return 8 * (((long long)B * S * Hkv + 7) / 8) * ((group + 3) / 4); }

// Workgroup `bid` of that grid: the units go to the XCDs round-robin by 3.23's decode rule -- unit = (idx / ngb) * 8 + xcd with xcd = bid & 7,
// idx = bid >> 3 -- so the ngb = ceil(group / 4) blocks of a unit stay on one XCD.  nd: the decode list's count, clamped to [0, B] by the caller.
// False for a workgroup past the last unit; else r < nd, c < S, hk < Hkv, gb < ngb.  (S, Hkv, group >= 1.)
SAGE_STEP_HD inline bool step_split_item(int bid, int nd, int S, int Hkv, int group, int &r, int &c, int &hk, int &gb)
{
    const int ngb = (group + 3) >> 2;
    const int xcd = bid & 7, idx = bid >> 3;
    const int uj = idx / ngb;
    gb = idx - uj * ngb;
    const long long unit = (long long)uj * 8 + xcd;
    if (bid < 0 || unit >= (long long)nd * S * Hkv) return false;
    const int rc = (int)(unit / Hkv);
    hk = (int)(unit - (long long)rc * Hkv);
    r = rc / S;
    c = rc - r * S;
    return true;
}

// the logical tiles chunk c of a sequence of `len` keys (clamped to [0, Lk] by the caller) may read: [t0, t1) = [c T, min((c + 1) T,
// ceil(len / 64))), empty (t1 <= t0) for a chunk at or behind ceil(len / 64) -- the only table entries a chunk's kernels look up
SAGE_STEP_HD inline void step_split_tile_range(int c, int T, int len, int &t0, int &t1)
{
    const long long a = (long long)c * T, e = a + T, nt = ((long long)(len > 0 ? len : 0) + 63) >> 6;
    t0 = (int)(a < 0x7fffffff ? a : 0x7fffffff);
    t1 = (int)(e < nt ? e : nt);
    if (t1 < t0) t1 = t0;
}

// row (b, kv head hk, chunk c, head gq of the group, row l) of chunk_max / lse_part [B, Hkv, S, group, lq_ws]; o_part holds D floats per row
SAGE_STEP_HD inline long long step_split_ws_row(int b, int hk, int c, int gq, int l, int Hkv, int S, int group, int lq_ws)
{
    return ((((long long)b * Hkv + hk) * S + c) * group + gq) * lq_ws + l;
}

}  // namespace sage
