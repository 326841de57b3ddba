"""CPU: tests/loop_plan.py -- the host model of a work item's loop partition -- against the definition of visibility, and what the GPU sweeps
chosen with it reach (tests/test_gpu_route_tile_counts.py, tests/test_gpu_route_random.py, tests/test_gpu_split_tile_counts.py,
tests/test_gpu_split_random.py).

The model restates the kernel's integer arithmetic, so it cannot vouch for itself.  For every work item of every sweep case the tile ranges are
recomputed here from ``ref_window.visible`` alone -- a boolean [rows, keys] matrix, no arithmetic of the kernel's:
  * the first 64-key tile in which a row of the query block sees a key is the model's ``kc0`` (windowed units; 0 elsewhere);
  * the last such tile, over the block's 128 row SLOTS (the kernel bounds the diagonal by the block, not by the rows a ragged block has), is
    tile ``kc0 / 64 + n_iters - 1``, and every tile a row that exists sees lies in the item's range;
  * the tiles of the range in which some existing row has a key in front of its window's left edge (visible without the window, not with
    it) are the model's ``nh`` head tiles.
A chunk of the kv_lens split (``split_chunk``) is checked the same way against the definition restricted to the chunk's keys.
The coverage sets are the sweeps' contract: they say which loop forms of which units the selection runs.
"""
import itertools

import numpy as np
import pytest

import loop_plan as lp
import ref_window as rw


def _tiles(mask):
    """Indices of the 64-key tiles in which the boolean [rows, keys] matrix has a True."""
    any_key = mask.numpy().any(axis=0) if mask.shape[0] else np.zeros(mask.shape[1], bool)
    return sorted({int(j) // 64 for j in np.nonzero(any_key)[0]})


def _agrees_with_visibility(p, causal, Lq, Lk, length, s, W, qblk):
    slots = lp.BLKQ * (qblk + 1)
    r0, r1 = lp.BLKQ * qblk, min(Lq, slots)
    if Lk == 0:
        assert p.n_iters == 0
        return
    s_def = s if causal else Lk                              # non-causal: every row's diagonal behind the last key
    keep = rw.visible(slots, Lk, s_def, W, 0, length)
    t_slots, t_rows = _tiles(keep[r0:slots]), _tiles(keep[r0:r1])
    what = (causal, Lq, Lk, length, s, W, qblk, p)
    first = p.kc0 // 64
    assert p.kc0 % 64 == 0 and (W > 0 or p.kc0 == 0), what
    assert all(first <= t < first + p.n_iters for t in t_rows), what
    if t_rows:
        assert t_rows[0] == first, what
    if t_slots:
        assert first + p.n_iters == t_slots[-1] + 1, what
        if r1 == slots:
            assert t_rows == t_slots, what
    else:
        assert p.n_iters <= 1, what                          # (a tile that holds the window's first key but only keys behind the length)
    cut = []
    if W > 0:
        left_of_window = rw.visible(slots, Lk, s_def, 0, 0, Lk) & ~rw.visible(slots, Lk, s_def, W, 0, Lk)
        cut = [t for t in _tiles(left_of_window[r0:r1]) if first <= t < first + p.n_iters]
        assert cut == list(range(first, first + len(cut))), what
    assert p.nh == len(cut), what
    # the partition itself: head tiles, then the pipelined run, then at least the two tiles the loop looks ahead (or the last-tile bodies)
    assert 0 <= p.nh <= p.n_iters and p.run == 6 * p.trips + p.remainder and 0 <= p.remainder < 6, what
    assert p.nh + p.run + (2 if p.run or p.diag_ok or p.tail_ok else 0) <= p.n_iters, what


# ---------------------------------------------------------------------------------------------- the model against visibility
@pytest.mark.parametrize("causal", [False, True])
def test_kv_lens_items_agree_with_visibility(causal):
    Lq = lp.LQ_CAUSAL_LENS if causal else lp.LQ
    for (n, j), p in lp.kv_lens_plans(causal).items():
        _agrees_with_visibility(p, causal, Lq, lp.LKP, n, 0, 0, j)


def test_q_start_items_agree_with_visibility():
    pairs = lp.Q_START_ALIGNED + lp.Q_START_PAIRS
    assert all(-lp.LQ <= s <= lp.LKP for _, s in pairs)     # (inside the kernel's clamp: the definition's offset is the kernel's)
    for (n, s, j), p in lp.q_start_plans(pairs).items():
        _agrees_with_visibility(p, True, lp.LQ, lp.LKP, n, s, 0, j)


def test_window_items_agree_with_visibility():
    assert all(s >= -lp.LQ and s - lp.LKP <= W for _, s, W in lp.window_cases())
    for lq in (lp.LQ,) + lp.PACK_LQS:
        for (n, s, W, j), p in lp.window_plans(lq).items():
            _agrees_with_visibility(p, True, lq, lp.LKP, n, max(s, -lq), W, j)      # (below -Lq no row sees a key either way: the kernel's clamp)


def test_pack_items_agree_with_visibility():
    for lq in lp.PACK_LQS:
        for (n,), p in lp.pack_plans("lens", lq).items():
            _agrees_with_visibility(p, False, lq, lp.LKP, n, 0, 0, 0)
        for (n, s), p in lp.pack_plans("qstart", lq).items():
            _agrees_with_visibility(p, True, lq, lp.LKP, n, max(s, -lq), 0, 0)      # (below -Lq no row sees a key either way)


def test_packed_items_agree_with_visibility():
    for (lq, lk, j), p in lp.packed_plans(0, lp.packed_br_pairs()).items():
        _agrees_with_visibility(p, True, lq, lk, lk, lk - lq, 0, j)
    for W, pairs in lp.packed_window_cases():
        for (lq, lk, j), p in lp.packed_plans(W, pairs).items():
            _agrees_with_visibility(p, True, lq, lk, lk, lk - lq, W, j)


def test_the_model_on_a_grid_of_offsets_and_windows():
    """Beyond the sweeps' own cases: every offset and window around the tile edges at a small shape, all three query blocks."""
    Lq, Lk = 300, 448
    for n, s, W in itertools.product((448, 400, 130, 64, 1), range(-310, 460, 21), (0, 1, 2, 63, 64, 65, 128, 200, 500)):
        for j in range(lp.nblk(Lq)):
            if W and s - Lk > W:
                continue                                     # (the kernel moves such offsets to Lk + W: no row sees a key either way)
            s2 = max(s, -Lq)                                 # (below -Lq no row sees a key either way: the kernel's clamp)
            _agrees_with_visibility(lp.dense(64, True, Lq, Lk, n, s2, W, j), True, Lq, Lk, n, s2, W, j)


# ---------------------------------------------------------------------------------------------- what the sweeps reach
def _forms(plans):
    return [p for p in plans.values() if p.exists and p.n_iters > 0]


def test_kv_lens_sweep_covers_every_trip_count_and_remainder():
    nc = _forms(lp.kv_lens_plans(False))
    # non-causal (the f8k units, TAIL_PIPE): the last-tile bodies run behind every run (tail_ok needs only two whole tiles), so the one place
    # without them is a sample of fewer than 128 keys, which runs no pipelined tile at all
    assert {(p.trips, p.remainder) for p in nc if p.tail_ok} >= set(lp.TRIPS_REM)
    assert {p.run for p in nc if p.tail_ok and p.n_iters - p.n_steady == 2} >= set(range(18))          # a whole last tile
    assert {p.run for p in nc if p.tail_ok and p.n_iters - p.n_steady == 3} >= set(range(18))          # a ragged one behind the two whole ones
    assert any(not p.tail_ok and p.run == 0 for p in nc)
    assert {n % 64 for n in lp.KV_LENS} == {0, 1, 63}
    c = _forms(lp.kv_lens_plans(True))
    assert {(p.trips, p.remainder, p.diag_ok) for p in c} >= set(itertools.product((0, 1, 2), range(6), (False, True)))


def test_q_start_sweep_covers_every_run_in_both_query_blocks():
    al = lp.q_start_plans(lp.Q_START_ALIGNED)
    assert all(s % 128 == 0 and s >= 0 for _, s in lp.Q_START_ALIGNED)
    assert {(p.trips, p.remainder) for p in _forms(al) if p.diag_ok} >= {(t, r) for t, r in lp.TRIPS_REM if (6 * t + r) % 2 == 0}
    pl = lp.q_start_plans(lp.Q_START_PAIRS)
    odd64 = {(j, p.run) for (n, s, j), p in pl.items() if s % 64 == 0 and s % 128 and p.diag_ok}
    assert odd64 >= {(0, r) for r in range(1, 18, 2)} | {(1, r) for r in range(1, 18, 2)}
    general3 = {(j, p.run) for (n, s, j), p in pl.items() if s % 64 and not p.diag_ok and p.n_iters - p.n_steady == 3}      # the diagonal across three general tiles
    assert general3 >= set(itertools.product((0, 1), range(18)))
    assert {(p.trips, p.remainder) for (n, s, j), p in pl.items() if s % 64} >= set(lp.TRIPS_REM)
    assert any(s < 0 and s % 64 for _, s in lp.Q_START_PAIRS) and any(s < 0 and s % 128 == 0 for _, s in lp.Q_START_PAIRS)
    assert any(not p.exists or p.n_iters == 0 for p in pl.values())                                    # blocks in front of key 0


def test_window_sweep_covers_head_tiles_times_runs():
    pl = lp.window_plans()
    forms = _forms(pl)
    assert {(p.nh, p.run) for p in forms} >= set(itertools.product(range(4), lp.RUNS))
    assert {(p.diag_ok, p.run > 0) for p in forms} >= {(False, True), (True, True)}
    edges = {s - W + j * lp.BLKQ + 1 - p.kc0 for (n, s, W, j), p in pl.items() if s - W + j * lp.BLKQ + 1 > 0 and p.nh > 0}
    assert edges >= {0, 1, 63}
    assert any(n < W and p.n_iters > 0 for (n, s, W, j), p in pl.items())                              # a sample shorter than its window
    assert any(s + j * lp.BLKQ - W + 1 >= n > 0 and p.exists for (n, s, W, j), p in pl.items())                                   # a window past the end of the keys
    assert len(lp.window_cases()) <= 48


def test_pack_sweep_covers_every_run_with_and_without_head_tiles():
    for lq in lp.PACK_LQS:
        assert {p.run for p in _forms(lp.pack_plans("window", lq)) if p.nh > 0} >= set(lp.RUNS), lq
        assert {p.run for p in _forms(lp.pack_plans("qstart", lq))} >= set(lp.RUNS), lq               # (no window: no head tiles)
        assert {(p.trips, p.remainder) for p in _forms(lp.pack_plans("lens", lq)) if p.tail_ok} >= set(lp.TRIPS_REM), lq


def test_packed_sweeps_cover_both_units():
    br = _forms(lp.packed_plans(0, lp.packed_br_pairs()))
    assert all(p.nh == 0 for p in br)
    assert {p.run for p in br} >= set(lp.RUNS) and {(p.trips, p.remainder) for p in br} >= set(lp.TRIPS_REM)
    assert {(p.diag_ok, p.run > 0) for p in br} >= {(False, True), (True, True)}
    win = [p for W, pairs in lp.packed_window_cases() for p in _forms(lp.packed_plans(W, pairs))]
    assert {(p.nh, p.run) for p in win} >= set(itertools.product(range(4), lp.RUNS))
    assert {(p.trips, p.remainder) for p in win} >= set(lp.TRIPS_REM)
    assert {(p.diag_ok, p.run > 0) for p in win} >= {(False, True), (True, True)}
    assert max(lk for _, lk in lp.packed_br_pairs()) <= lp.LKP and max(lk for _, pairs in lp.packed_window_cases() for _, lk in pairs) <= lp.LKP


# ---------------------------------------------------------------------------------------------- the random generator
def test_random_calls_mostly_see_keys():
    """Conditioning on the draw: a call whose every row sees no key checks nothing.  At least 95 of the first 100 seeds have a sample in which at
    least half the rows see a key; every kind of offset and window, and pack_gqa, are drawn among them."""
    good, kinds = 0, set()
    for seed in range(100):
        c = lp.random_call(seed)
        assert c["D"] in (64, 128, 96) and 1 <= c["B"] <= 3 and 1 <= c["Hkv"] <= 2 and c["group"] in (1, 2, 4) and 1 <= c["Lq"] <= 420
        assert c["Lk"] <= lp.LKP and all(0 <= n <= c["Lk"] for n in c["lens"]) and (not c["pack_gqa"] or (c["Lq"] <= 32 and c["group"] >= 2))
        share = []
        for n, s, ws, causal in lp.random_call_geometry(c):
            assert -c["Lq"] - 5 <= s <= c["Lk"] + 5 or c["causal_align"] == "bottom_right"
            share.append(float(rw.visible_from_keywords(c["Lq"], c["Lk"], ws, causal, s, n).any(dim=1).float().mean()))
        good += max(share) >= 0.5
        q = c["q_start"]
        kinds.add(("offset", "bottom_right" if c["causal_align"] != "top_left" else "none" if q is None else "int" if isinstance(q, int) else "tensor"))
        kinds.add(("window", "none" if c["window_size"] is None else "causal" if c["is_causal"] else "two_sided"))
        kinds.add(("pack", c["pack_gqa"]))
    assert good >= 95, good
    assert len(kinds) == 4 + 3 + 2, kinds


# ---------------------------------------------------------------------------------------------- num_splits: a chunk of the kv_lens split
def _chunk_agrees_with_visibility(p, causal, Lq, Lkp, length, s, S, chunk):
    """``split_chunk`` against the definition restricted to the chunk's keys [kc0, kc0 + 64 T): the chunk's tile range over the block's 128 row
    slots and over the rows that exist, in the chunk's own tile numbers."""
    T = lp.split_tiles(Lkp, S)
    what = (causal, Lq, Lkp, length, s, S, chunk, p)
    assert p.kc0 == chunk * 64 * T and p.nh == 0 and p.exists, what
    s_def = max(-Lq, min(s, Lkp)) if causal else Lkp          # (the kernel's clamp: outside it no row's keys change; non-causal: every diagonal behind the last key)
    keep = rw.visible(lp.BLKQ, Lkp, s_def, 0, 0, length)[:, p.kc0:p.kc0 + 64 * T]
    t_slots, t_rows = _tiles(keep), _tiles(keep[:Lq])
    n_keys = int(keep.any(dim=0).sum()) if not causal else None
    if not causal:
        assert p.lk == n_keys, what                          # the chunk's keys in front of len_b
    assert p.lk == max(0, min(max(0, min(length, Lkp)) - p.kc0, 64 * T)), what
    assert all(0 <= t < p.n_iters for t in t_rows), what
    if t_rows:
        assert t_rows[0] == 0, what                          # visibility is a prefix of the keys: a chunk a row reaches, it reaches from its first key
    assert p.n_iters == (t_slots[-1] + 1 if t_slots else 0), what
    if Lq == lp.BLKQ:
        assert t_rows == t_slots, what
    assert p.run == 6 * p.trips + p.remainder and 0 <= p.remainder < 6, what
    assert p.run + (2 if p.run or p.diag_ok or p.tail_ok else 0) <= p.n_iters, what
    # the steady tiles are whole tiles in front of len_b that every row slot sees whole (no mask of either kind)
    if p.run:
        whole = rw.visible(lp.BLKQ, Lkp, s_def, 0, 0, length)[:, p.kc0:p.kc0 + 64 * p.run]
        assert bool(whole.all()), what


def test_split_chunks_agree_with_visibility_on_the_tables():
    for lq in lp.SPLIT_LQS:
        for (n, s, c), p in lp.split_plans(False, lq, lp.SPLIT_LENS).items():
            _chunk_agrees_with_visibility(p, False, lq, lp.LKP_SPLIT, n, 0, lp.S_SPLIT, c)
        for (n, s, c), p in lp.split_plans(True, lq, lp.split_causal_pairs()).items():
            _chunk_agrees_with_visibility(p, True, lq, lp.LKP_SPLIT, n, s, lp.S_SPLIT, c)
    for Lkp, S, lens, pairs in lp.SPLIT_COUNT_CASES:
        for lq in (1, 33, 128):
            for (n, s, c), p in lp.split_plans(False, lq, lens, Lkp, S).items():
                _chunk_agrees_with_visibility(p, False, lq, Lkp, n, 0, S, c)
            for (n, s, c), p in lp.split_plans(True, lq, pairs, Lkp, S).items():
                _chunk_agrees_with_visibility(p, True, lq, Lkp, n, s, S, c)


def test_split_chunks_on_a_grid_of_lengths_offsets_and_counts():
    """Beyond the tables: lengths and offsets around the tile and chunk edges at a small padded length (449 keys: 8 tiles, the last of one key),
    every chunk of S = 2, 3, 5, 8 and 11 -- chunks past len_b, behind the diagonal and past the tensor (S = 5: T = 2, chunk 4 starts at the
    tensor's end; S = 11: T = 1, three chunks past it) among them -- non-causal and causal."""
    Lkp = 449
    seen = set()
    for S, lq in itertools.product((2, 3, 5, 8, 11), (1, 33, 128)):
        T = lp.split_tiles(Lkp, S)
        for n in (449, 448, 400, 385, 384, 257, 256, 130, 64, 63, 1, 0, -4, 500):
            for c in range(S):
                _chunk_agrees_with_visibility(lp.split_chunk(False, lq, Lkp, n, None, S, c), False, lq, Lkp, n, 0, S, c)
                for s in range(-140, 470, 19):
                    p = lp.split_chunk(True, lq, Lkp, n, s, S, c)
                    _chunk_agrees_with_visibility(p, True, lq, Lkp, n, s, S, c)
                    seen.add("past_len" if p.lk == 0 and 0 < n and c * 64 * T < Lkp else "past_tensor" if c * 64 * T >= Lkp else
                             "behind_diagonal" if p.n_iters == 0 else "work")
    assert seen == {"past_len", "past_tensor", "behind_diagonal", "work"}


def _split_reach(plans):
    return [p for p in plans.values() if p.lk > 0 and p.n_iters > 0]


def test_split_tables_cover_every_trip_count_and_remainder_in_both_chunks():
    """The conditions of the sweep of num_splits (tests/test_gpu_split_tile_counts.py), at every Lq of the packed and the unpacked form."""
    assert lp.split_tiles(lp.LKP_SPLIT, lp.S_SPLIT) == 20
    for lq in lp.SPLIT_LQS:
        for causal, cases in ((False, lp.SPLIT_LENS), (True, lp.split_causal_pairs())):
            plans = lp.split_plans(causal, lq, cases)
            forms = _split_reach(plans)
            for chunk in range(lp.S_SPLIT):
                got = {(p.trips, p.remainder) for (n, s, c), p in plans.items() if c == chunk and p.lk > 0 and p.n_iters > 0}
                assert got >= set(lp.TRIPS_REM), (lq, causal, chunk, sorted(set(lp.TRIPS_REM) - got))
            last = {((p.diag_ok if causal else p.tail_ok), p.run > 0) for p in forms}
            assert last >= {(True, True), (True, False)} | ({(False, True)} if causal else set()), (lq, causal, last)
            assert any(p.lk == 0 and n > 0 for (n, s, c), p in plans.items()), (lq, causal)                 # a chunk past len_b
            assert any(0 < p.lk < 64 and p.n_iters == 1 for p in plans.values()), (lq, causal)              # exactly one ragged tile
            if causal:
                assert any(p.lk > 0 and p.n_iters == 0 for p in plans.values()), lq                         # a chunk behind the diagonal
                # every run in front of the pipelined diagonal bodies (aligned offsets) and in front of general tiles (any other)
                got = {(c, p.trips, p.remainder, p.diag_ok) for (n, s, c), p in plans.items() if p.lk > 0 and p.n_iters > 0}
                assert got >= {(c, t, r, d) for c in range(lp.S_SPLIT) for t, r in lp.TRIPS_REM for d in (False, True)}, lq
    # non-causal: chunk 0 and chunk 1 as a partial chunk of every whole-tile count with a whole and with a ragged last tile; chunk 1 empty
    nc = lp.split_plans(False, 1, lp.SPLIT_LENS)
    for chunk in range(2):
        assert {(p.lk // 64, p.lk % 64) for (n, s, c), p in nc.items() if c == chunk} >= {(t, e) for t in range(20) for e in (0, 1, 63)} | {(20, 0)}
    assert any(p.lk == 0 for (n, s, c), p in nc.items() if c == 1 and n == 1280)
    # causal: offsets of every kind
    pairs = lp.split_causal_pairs()
    assert all(p in pairs for p in lp.SPLIT_CAUSAL_SPECIAL)
    assert any(s < 0 for n, s in pairs) and any(s >= n > 0 for n, s in pairs) and any(n == 0 for n, s in pairs)
    assert {s - lp.LKP_SPLIT // 2 for n, s in pairs} >= {-1, 0, 1}                                          # row 0's diagonal on the chunk boundary
    assert any(s == n - lq for n, s in pairs for lq in lp.SPLIT_LQS) and any(s % 64 == 0 for n, s in pairs) and any(s % 64 for n, s in pairs)
    assert len(pairs) <= 128, len(pairs)                                                                    # (one call carries the table)


def test_split_count_cases_reach_the_chunk_counts():
    got = {(Lkp, S, lp.split_tiles(Lkp, S)) for Lkp, S, _, _ in lp.SPLIT_COUNT_CASES}
    assert got == {(2560, 40, 1), (2560, 20, 2), (2560, 13, 4), (2560, 255, 1), (2561, 3, 14)}
    for Lkp, S, lens, pairs in lp.SPLIT_COUNT_CASES:
        T, nt = lp.split_tiles(Lkp, S), (Lkp + 63) // 64
        assert Lkp in lens and any(n % 64 for n in lens) and 0 in lens
        assert ((S - 1) * T >= nt) == ((Lkp, S) in ((2560, 13), (2560, 255)))                                      # trailing chunks past the tensor
        for causal, cases in ((False, lens), (True, pairs)):
            plans = lp.split_plans(causal, 33, cases, Lkp, S)
            assert all(p.lk == 0 for (n, s, c), p in plans.items() if c * 64 * T >= Lkp)
            assert any(p.lk > 0 and p.n_iters > 0 for (n, s, c), p in plans.items() if c == min(S, -(-nt // T)) - 1)      # the tensor's last chunk runs
    assert sum(1 for _, S, _, _ in lp.SPLIT_COUNT_CASES if S == 255) == 1 and 255 * 1 - 40 == 215


# ---------------------------------------------------------------------------------------------- the random generator of num_splits
def test_random_calls_draw_what_they_drew():
    """``random_call`` keeps its own stream (seed 31000 + seed) beside the second generator: its first draws are that stream's first, it draws no
    chunk count, and it is a function of the seed alone."""
    import random
    for seed in (0, 41, 99):
        rng = random.Random(31000 + seed)
        c = lp.random_call(seed)
        assert (c["D"], c["dtype"], c["layout"]) == (rng.choice((64, 128, 96)), rng.choice(("f16", "bf16")), rng.choice(("HND", "NHD")))
        assert "S" not in c and lp.random_call(seed) == c
    drawn = {s: (c["D"], c["Lq"], c["Lk"], tuple(c["lens"]), c["pack_gqa"]) for s, c in ((s, lp.random_call(s)) for s in (0, 41, 99))}
    assert drawn == {0: (128, 102, 705, (705, 699, 412), False), 41: (96, 304, 1216, (352, 1216, 735), False), 99: (64, 18, 128, (92,), False)}      # (as before the second generator)


def test_random_split_calls_mostly_see_keys():
    """test_random_calls_mostly_see_keys for ``random_split_call``: at least 95 of the first 100 seeds have a sample in which at least half the
    rows see a key; every chunk count of the list, every kind of offset and pack_gqa are drawn."""
    good, kinds = 0, set()
    for seed in range(100):
        c = lp.random_split_call(seed)
        assert c["D"] in (64, 128, 96) and 1 <= c["B"] <= 3 and 1 <= c["Hkv"] <= 2 and c["group"] in (1, 2, 4, 5) and 1 <= c["Lq"] <= 128
        assert c["Lk"] <= lp.LKP_SPLIT and all(0 <= n <= c["Lk"] for n in c["lens"]) and (not c["pack_gqa"] or (c["Lq"] <= 32 and c["group"] >= 2))
        assert 2 <= c["S"] <= 255 and c["window_size"] is None and c["is_causal"] == (c["offset"] != "none")
        tiles = (c["Lk"] + 63) // 64
        assert c["S"] == max(2, {"tiles": tiles, "tiles+3": tiles + 3}.get(c["S_kind"]) or int(c["S_kind"]))
        share = []
        for n, s, ws, causal in lp.random_call_geometry(c):
            assert -c["Lq"] - 5 <= s <= c["Lk"] + 5 or c["causal_align"] == "bottom_right"
            share.append(float(rw.visible_from_keywords(c["Lq"], c["Lk"], ws, causal, s, n).any(dim=1).float().mean()))
        good += max(share) >= 0.5
        kinds.add(("offset", c["offset"]))
        kinds.add(("S", c["S_kind"]))
        kinds.add(("pack", c["pack_gqa"]))
    assert good >= 95, good
    assert kinds == {("offset", o) for o in lp.SPLIT_RANDOM_OFFSETS} | {("S", k) for k in lp.SPLIT_RANDOM_S} | {("pack", False), ("pack", True)}, kinds
    assert lp.random_split_call(7) == lp.random_split_call(7)
