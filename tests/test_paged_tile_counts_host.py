"""CPU: what the case tables of the paged tile-count sweep (tests/test_gpu_paged_tile_counts.py) reach, computed from the tables with the host
model of the loop partition (tests/loop_plan.py, itself pinned against the definition of visibility in tests/test_loop_plan_host.py).

A set asserted here is the claim of the GPU file's docstring: the loop forms every one of the six paged compilation units runs at least once,
per head size (the tables do not depend on it), in a call that is compared bit for bit with its sibling route."""
import loop_plan as lp

TRIPS_REM = set(lp.TRIPS_REM)
RUNS15, RUNS18 = set(lp.RUNS), set(lp.PAGED_RUNS)


def _ran(plans):
    return [p for p in plans if p.n_iters > 0]


def test_the_shared_samples():
    lens = [n for n, _ in lp.PAGED_SAMPLES]
    assert len(lp.PAGED_SAMPLES) == 111 and max(lens) == lp.LKP == 24 * 64 and min(lens) == 0
    assert {n % 64 for n in lens} >= {0, 1, 63}                                      # a whole last tile and ragged ones
    assert any(s < 0 for _, s in lp.PAGED_SAMPLES) and any(s % 64 == 0 for _, s in lp.PAGED_SAMPLES) and any(s % 64 for _, s in lp.PAGED_SAMPLES)


def test_f8p_non_causal_every_trip_and_remainder_behind_the_tail_bodies():
    plans = _ran(lp.paged_plans(lp.LQ, False).values())
    assert {(p.trips, p.remainder) for p in plans if p.tail_ok} >= TRIPS_REM
    assert {p.lk % 64 == 0 for p in plans if p.tail_ok and p.run > 0} == {True, False}        # the last tile whole and ragged
    assert any(not p.entered for p in plans)                                                      # one and two tiles: general iterations only


def test_f8p_causal_every_run_in_front_of_both_kinds_of_diagonal():
    plans = lp.paged_plans(lp.LQ, True)
    for j in range(lp.nblk(lp.LQ)):                                                  # in the whole query block and in the ragged one
        got = {(p.run, p.diag_ok) for (b, jj), p in plans.items() if jj == j and p.n_iters}
        assert got >= {(r, d) for r in RUNS18 for d in (False, True)}, (j, sorted({(r, d) for r in RUNS18 for d in (False, True)} - got))
    # aligned and unaligned offsets; rows in front of key 0; a sample without keys
    assert any(p.diag_ok and p.kchunk0 % 64 == 0 for p in plans.values()) and any(p.n_iters and p.kchunk0 % 64 for p in plans.values())
    assert any(p.n_iters == 0 for p in plans.values())


def test_the_windows_reach_every_head_tile_count_and_run():
    ws = lp.paged_windows()
    assert 8 <= len(ws) <= 16, ws                                                    # one call per window and route: a dozen, not the product
    form, pack, diag = set(), set(), set()
    for W in ws:
        for p in _ran(lp.paged_plans(lp.LQ, True, W).values()):
            form.add((p.nh, p.run))
            diag.add((p.diag_ok, p.run > 0))
        for lq in lp.PACK_LQS:
            pack |= {(lq, p.run) for p in _ran(lp.paged_plans(lq, True, W).values()) if p.nh > 0}
    assert form >= {(nh, r) for nh in range(4) for r in RUNS15}                      # f8p: head tiles {0, 1, 2, 3} x run 0 .. 14
    assert pack >= {(lq, r) for lq in lp.PACK_LQS for r in RUNS15}                   # f8pg: every run behind head tiles
    assert diag >= {(True, True), (False, True)}


def test_f8pg_every_trip_remainder_and_run():
    for lq in lp.PACK_LQS:
        assert {(p.trips, p.remainder) for p in _ran(lp.paged_plans(lq, False).values()) if p.tail_ok} >= TRIPS_REM, lq
        assert {p.run for p in _ran(lp.paged_plans(lq, True).values()) if p.nh == 0} >= RUNS18, lq      # without head tiles


def test_f8pks_every_trip_and_remainder_in_a_chunk_and_a_chunk_that_starts_inside_a_page():
    assert lp.paged_split_samples()[:len(lp.SPLIT_LENS)] == tuple((n, n - 128) for n in lp.SPLIT_LENS) and len(lp.paged_split_samples()) <= 256
    assert [lp.split_tiles(lp.LKP_SPLIT, S) for S in lp.PAGED_SPLITS] == [20, 14, 8]
    # pages of 256 keys hold four tiles: with S 3 chunk 1 starts at tile 14 = tile 2 of page 3, and chunk 2 (tiles 28 .. 41) ends behind the table
    assert 14 % 4 == 2 and 3 * 14 > lp.LKP_SPLIT // 64 and 20 % 4 == 0 and 8 % 4 == 0
    for causal in (False, True):
        for lq in lp.PAGED_SPLIT_LQS:
            for S, most in ((2, TRIPS_REM), (3, {(t, r) for t, r in TRIPS_REM if 6 * t + r <= 12}), (5, {(t, r) for t, r in TRIPS_REM if 6 * t + r <= 6})):
                plans = lp.paged_split_plans(causal, lq, S)
                for c in range(S - 1 if S == 3 else S):                             # (S 3: the last chunk holds 12 tiles of the table's 40)
                    got = {(p.trips, p.remainder) for (b, cc), p in plans.items() if cc == c and p.lk and p.n_iters}
                    assert got >= most, (causal, lq, S, c, sorted(most - got))
                last = {(p.trips, p.remainder) for (b, cc), p in plans.items() if cc == S - 1 and p.lk and p.n_iters}
                assert S != 3 or last >= {(t, r) for t, r in TRIPS_REM if 6 * t + r <= 10}
                if causal:
                    assert {p.diag_ok for p in plans.values() if p.lk and p.n_iters and p.run > 0} == {True, False}
                assert any(p.lk == 0 for p in plans.values()) and any(0 < p.lk < 64 for p in plans.values())      # chunks past len_b, one ragged tile


def test_ragged_and_step_every_trip_and_remainder_in_every_band():
    assert sorted(lp.PAGED_RAGGED_LQS) == [1, 32, 33, 128, 130] and lp.PAGED_ROTATIONS == 5
    for b in range(len(lp.PAGED_SAMPLES)):                                           # over the rotations every sample takes every row count
        assert {lp.paged_ragged_counts(r)[b] for r in range(lp.PAGED_ROTATIONS)} == set(lp.PAGED_RAGGED_LQS)
    for bottom_right in (False, True):
        reach = {band: set() for band in lp.PAGED_BANDS}
        diag = {band: set() for band in lp.PAGED_BANDS}
        for r in range(lp.PAGED_ROTATIONS):
            for band, p in lp.paged_ragged_plans(r, 0, bottom_right).values():
                if p.n_iters:
                    reach[band].add((p.trips, p.remainder))
                    diag[band].add(p.diag_ok)
        for band in lp.PAGED_BANDS:                                                  # run 0 .. 17: every trip x remainder, and so every run 0 .. 14
            assert reach[band] >= TRIPS_REM, (bottom_right, band, sorted(TRIPS_REM - reach[band]))
            # (bottom-right the diagonal ends on the last key, whose tile is whole for none of these lengths and row counts: general iterations;
            #  the pipelined diagonal bodies are the explicit offsets')
            assert diag[band] == {True, False} or bottom_right, (bottom_right, band)
    # under the windows: head tiles in front of a pipelined run in every band
    heads = {band: set() for band in lp.PAGED_BANDS}
    for i, W in enumerate(lp.paged_windows()):
        for band, p in lp.paged_ragged_plans(i % lp.PAGED_ROTATIONS, W).values():
            if p.n_iters and p.nh > 0:
                heads[band].add(p.run)
    for band in lp.PAGED_BANDS:
        assert len(heads[band] - {0}) >= 6, (band, sorted(heads[band]))


def test_every_unit_has_a_sample_for_the_attention_reference():
    """The anchors of the GPU file, selected as it selects them: two trips and a remainder, keys to see."""
    picks = [lp.paged_window_anchor()[1:], lp.paged_anchor(lp.paged_plans(16, True))]
    assert picks[0][1].nh > 0
    split = lp.paged_split_plans(True, 16, 2)
    picks.append(lp.paged_anchor(split, key=lambda kk: kk[1] == 1 and split[kk[0], 0].n_iters > 0))
    picks += [lp.paged_ragged_anchor(band)[1:] for band in ("two0", "decode", "chunk")]
    for b, p in picks:
        assert p.trips >= 2 and p.remainder > 0 and p.lk >= 14 * 64, (b, p)
