"""A host model of ONE work item's loop partition in the FP8-PV attention kernel -- TEST INFRASTRUCTURE ONLY.

``csrc/sage_attn_kernel.h`` decides with integer arithmetic which loop forms a work item (one 128-row query block of one head) runs: head
tiles (WINDOW: general iterations that cut some row on the left), the six-body pipelined loop (``csrc/sage_attn_loop_f8.h``: ``trips`` times six
bodies, then ``remainder`` single bodies renamed behind them), the last-tile bodies (``diag_ok`` causal, ``tail_ok`` non-causal) and general
iterations.  This module restates that arithmetic in plain Python -- C's truncating division included -- so that the GPU sweeps
(tests/test_gpu_route_tile_counts.py, tests/test_gpu_split_tile_counts.py, tests/test_gpu_paged_tile_counts.py) can CHOOSE lengths, offsets and windows by the loop forms they reach and ASSERT what the selection
covers.  It is not a reference for values, and it imports nothing from ``sageattention_amd``.  tests/test_loop_plan_host.py pins it on the
CPU against tile ranges recomputed from the definition of visibility (``ref_window.visible``).

The second half holds the case tables of the sweeps: pure data and greedy selections over this model, shared by the host test and the GPU
tests.
"""
from __future__ import annotations

import collections
import functools
import itertools

BLKQ, BLKK = 128, 64
W_MAX = 1 << 30

Plan = collections.namedtuple("Plan", "exists kc0 lk n_iters nh n_steady diag_ok tail_ok entered run trips remainder kchunk0")


def _tdiv(a: int, b: int) -> int:
    """C's integer division: truncation towards zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _item(causal: bool, Lq: int, Lk: int, qstart, W: int, qblk: int, kc0: int = 0) -> Plan:
    """The kernel's bounds behind its per-route clamps.  ``Lk``: the item's key count (before the window's shift); ``qstart``: None without
    QSTART; ``W``: 0 without WINDOW (else >= 1, already clamped); ``kc0``: the item's first key where the route and not the window sets it (a
    chunk of the kv_lens split), a multiple of 64."""
    exists = qblk * BLKQ < Lq
    assert kc0 % BLKK == 0 and not (W and kc0)
    if W:
        a0 = (qstart - W) + qblk * BLKQ + 1
        kc0 = (a0 & ~(BLKK - 1)) if a0 > 0 else 0
        Lk = Lk - kc0 if Lk > kc0 else 0
    kchunk0 = kc0 - qstart if qstart is not None else 0
    n_iters = _tdiv(Lk + BLKK - 1, BLKK)
    if causal:
        lim = max(_tdiv(qblk * BLKQ + BLKQ - kchunk0 + BLKK - 1, BLKK), 0)
        n_iters = min(lim, n_iters)
    nh = 0
    if W:
        rlast = min(qblk * BLKQ + BLKQ - 1, Lq - 1)
        x = rlast - kchunk0 + 1 - W
        nh = min((x + BLKK - 1) >> 6 if x > 0 else 0, n_iters)
    n_steady = min(_tdiv(Lk, BLKK) - 2, n_iters - 2)
    if causal:
        n_steady = min(n_steady, max(_tdiv(qblk * BLKQ - kchunk0, BLKK), 0))
    diag_ok = causal and (qstart is None or (kchunk0 & (BLKK - 1)) == 0) and \
        ((n_iters - n_steady == 2) if n_steady > 0 else (n_iters == 2 and Lk >= 2 * BLKK))
    if W:
        diag_ok = diag_ok and nh <= max(n_steady, 0)
    tail_ok = (not causal) and n_steady == _tdiv(Lk, BLKK) - 2 and n_steady >= 0 and n_iters - n_steady <= 3
    it0 = nh                                              # the pipelined loop enters behind the head tiles
    entered = it0 < n_steady or diag_ok or tail_ok
    left = n_steady - it0 if entered else 0
    run = max(left, 0)
    return Plan(exists, kc0, Lk, n_iters, nh, n_steady, diag_ok, tail_ok, entered, run, run // 6, run % 6, kchunk0)


def dense(D: int, causal: bool, Lq: int, Lk_padded: int, len_b: int, s_b, W: int, qblk: int) -> Plan:
    """A dense launch of the KVLEN kernels.  ``s_b`` None: no offsets (non-causal, or the top-left diagonal); ``W`` 0: no window, else the
    number of keys a row sees up to and including its diagonal (``window_size=(W - 1, 0)``).  ``D`` selects no bound of the FP8-PV units (both
    head sizes run the six-body loop and the last-tile bodies); it is an input so that a case names its unit."""
    assert D in (64, 128) and (s_b is None or causal) and (W == 0 or s_b is not None)
    Lk = max(0, min(len_b, Lk_padded))
    qstart = None
    if s_b is not None:
        if W:
            W = 1 if W < 1 else min(W, W_MAX)
            sl = max(s_b, -Lq)
            qstart = Lk_padded + W if sl - Lk_padded > W else sl
        else:
            qstart = max(-Lq, min(s_b, Lk_padded))
    return _item(causal, Lq, Lk, qstart, W, qblk)


def packed(Lq_b: int, Lk_b: int, W: int, qblk: int, D: int = 128) -> Plan:
    """A sequence of a packed bottom-right launch (``s_b = Lk_b - Lq_b``, never clamped); ``W`` 0: no window (the ``f8vb`` units), else the
    ``f8vbw`` units."""
    if W:
        W = 1 if W < 1 else min(W, W_MAX)
    return _item(True, Lq_b, Lk_b, Lk_b - Lq_b, W, qblk)


def split_tiles(Lk_padded: int, S: int) -> int:
    """T, the 64-key tiles of a chunk of the kv_lens split: ceil(ceil(Lk_padded / 64) / S)."""
    nt = (Lk_padded + BLKK - 1) // BLKK
    return (nt + S - 1) // S


def split_chunk(causal: bool, Lq: int, Lk_padded: int, len_b: int, s_b, S: int, chunk: int) -> Plan:
    """Chunk ``chunk`` of pass 2 of the kv_lens split (``num_splits=S``, the ``f8ks`` units; SEED with KVLEN in ``csrc/sage_attn_kernel.h``): a
    call of one query block on keys [kc0, kc0 + 64 T) of the sample's first ``len_b``.  The length and the offset are formed as the KVLEN /
    QSTART kernels form them and shifted into the chunk: Lk = clamp(len_b - kc0, 0, 64 T), kchunk0 = kc0 - qstart.  ``s_b``: the offset of a
    causal call (0: top-left), ignored without ``causal``.  No window, one query block."""
    assert 1 <= Lq <= BLKQ and 2 <= S <= 255 and 0 <= chunk < S and (s_b is not None or not causal)
    T = split_tiles(Lk_padded, S)
    kc0 = chunk * BLKK * T
    lenb = max(0, min(len_b, Lk_padded))
    lk = max(0, min(lenb - kc0, BLKK * T))
    qstart = max(-Lq, min(s_b, Lk_padded)) if causal else None
    return _item(causal, Lq, lk, qstart, 0, 0, kc0)


def nblk(Lq: int) -> int:
    return (Lq + BLKQ - 1) // BLKQ


def describe(p: Plan) -> str:
    return f"(nh {p.nh}, run {p.run}, trips {p.trips}, rem {p.remainder}, diag_ok {int(p.diag_ok)}, tail_ok {int(p.tail_ok)})"


# ================================================================================================ the case tables of the sweeps
LQ, LKP = 200, 1536                       # one whole and one ragged query block; 24 key tiles
LQ_CAUSAL_LENS = 1224                     # sweep (a), causal top-left: see KV_LENS below
RUNS = tuple(range(15))                   # the pipelined-run lengths every sweep reaches
TRIPS_REM = tuple(itertools.product((0, 1, 2), range(6)))
PACK_LQS, PACK_GROUPS = (1, 16, 32), (4, 5)


def _greedy(candidates, keys_of, wanted):
    """A cover of ``wanted``: again and again the candidate that reaches most of what is still missing (the first of equals)."""
    missing, picked = set(wanted), []
    reach = [(c, keys_of(c) & missing) for c in dict.fromkeys(candidates)]
    while missing:
        reach = [(c, k & missing) for c, k in reach if k & missing]
        assert reach, sorted(missing, key=repr)[:8]
        c, k = max(reach, key=lambda ck: len(ck[1]))
        picked.append(c)
        missing -= k
    return tuple(picked)


# ---- (a) kv_lens: every count of whole tiles 0 .. 20 with a whole last tile and with tails of 1 and 63 keys, and the full 24 tiles.
# Non-causal, the run is len // 64 - 2 in both query blocks.  Causal top-left, the diagonal caps it at 2 qblk, so Lq = 200 could reach a run
# of 2 at the most: the causal sweep takes Lq = 1224 (nine whole query blocks and a ragged one), where block qblk runs min(len // 64 - 2, 2 qblk).
KV_LENS = tuple(sorted({0, LKP} | {64 * t + e for t in range(21) for e in (0, 1, 63)}))


def kv_lens_plans(causal: bool):
    Lq = LQ_CAUSAL_LENS if causal else LQ
    return {(n, j): dense(128, causal, Lq, LKP, n, None, 0, j) for n in KV_LENS for j in range(nblk(Lq))}


# ---- (b) q_start: (len, offset).  Offset 64 k + e puts 2 qblk + k steady tiles in front of the diagonal of block qblk; e = 0 keeps the
# pipelined diagonal bodies, any other e puts the diagonal across three general tiles.  k = -2 .. 17 reaches every run 0 .. 17 in both blocks.
Q_START_ALIGNED = tuple((LKP, 128 * k) for k in range(0, 9)) + ((900, 640),)                       # multiples of 128 (>= 0: the padded plain call)
Q_START_PAIRS = tuple((LKP, 64 * k + (1, 37, 63)[(k + 2) % 3]) for k in range(-2, 18)) + tuple((LKP, 64 * k) for k in range(-1, 18, 2)) + \
    ((LKP, -128), (LKP, -199), (700, 500), (1000, 930), (1100, 1100 - LQ), (65, -70), (0, 5))


def q_start_plans(pairs):
    return {(n, s, j): dense(128, True, LQ, LKP, n, s, 0, j) for n, s in pairs for j in range(nblk(LQ))}


# ---- (c) window_size: (len, offset, W), chosen greedily from a grid by what the model says they reach
def _window_candidates():
    lens = (LKP, 1500)
    for k in range(-2, 19):
        for e in (0, 1, 37, 63):
            s = 64 * k + e
            ws = [64 * m + d for m in range(0, 21) for d in (0, 1, 37) if 64 * m + d >= 1]
            ws += [s + c for c in (1, 60, 130, 150, 190, 200, 260) if s + c >= 1]
            for i, W in enumerate(ws):
                yield (lens[(k + i) & 1], s, W)


def _window_keys(case, lq=LQ):
    n, s, W = case
    keys = set()
    for j in range(nblk(lq)):
        p = dense(128, True, lq, LKP, n, s, W, j)
        if p.n_iters == 0:
            continue
        keys.add(("form", p.nh, p.run))
        keys.add(("diag", p.diag_ok, p.run > 0))
        a0 = s - W + j * BLKQ + 1
        if a0 > 0 and p.nh > 0:
            keys.add(("edge", a0 - p.kc0))
    for lq_p in PACK_LQS:                                 # the same table serves the packed decode launch (d)
        p = dense(128, True, lq_p, LKP, n, s, W, 0)
        if p.n_iters and p.nh > 0:
            keys.add(("pack", lq_p, p.run))
    return keys


WINDOW_WANTED = {("form", nh, r) for nh in range(4) for r in RUNS} | {("diag", d, True) for d in (False, True)} | \
    {("edge", e) for e in (0, 1, 63)} | {("pack", lq, r) for lq in PACK_LQS for r in RUNS}
# a sample shorter than its window (every row sees all 100 keys or none); a window past the end of the keys (block 1 sees nothing, block 0 the
# last keys); a sample without keys
WINDOW_SPECIAL = ((100, -50, 300), (300, 350, 100), (0, 5, 64))


@functools.lru_cache(maxsize=None)
def window_cases():
    return _greedy(_window_candidates(), _window_keys, WINDOW_WANTED) + WINDOW_SPECIAL


def window_plans(lq=LQ):
    return {(n, s, W, j): dense(128, True, lq, LKP, n, s, W, j) for n, s, W in window_cases() for j in range(nblk(lq))}


# ---- (d) pack_gqa: the tables above at Lq in {1, 16, 32} (one query block: qblk = 0)
def pack_plans(route: str, lq: int):
    if route == "lens":
        return {(n,): dense(128, False, lq, LKP, n, None, 0, 0) for n in KV_LENS}
    if route == "qstart":
        return {(n, s): dense(128, True, lq, LKP, n, s, 0, 0) for n, s in Q_START_ALIGNED + Q_START_PAIRS}
    assert route == "window"
    return {(n, s, W): dense(128, True, lq, LKP, n, s, W, 0) for n, s, W in window_cases()}


# ---- (e) the packed launches: (Lq_b, Lk_b) for bottom-right, (W, Lq_b, Lk_b) for the window
def _packed_keys(case):
    W, lq, lk = case
    keys = set()
    for j in range(nblk(lq)):
        p = packed(lq, lk, W, j)
        if p.n_iters == 0:
            continue
        keys.add(("form", p.nh, p.run))
        keys.add(("loop", p.trips, p.remainder))
        keys.add(("diag", p.diag_ok, p.run > 0))
    return keys


def _packed_br_candidates():
    for lq in (200, 128, 72, 1, 16):
        for t in range(0, 22):
            for e in (0, 1, 37):
                lk = lq + 64 * t + e
                if lk <= LKP:
                    yield (0, lq, lk)


def _packed_window_candidates():
    for lq in (1, 40, 128, 200):
        for m in range(0, 21):
            for d in (0, 1, 37, 63):
                W = 64 * m + d
                if W < 1:
                    continue
                for lk in (W + 64 * a + c for a in (0, 1, 4, 6) for c in (0, 5, -30, 64 - d)):
                    if 1 <= lk <= LKP:
                        yield (W, lq, lk)
        for lk in range(64, LKP + 1, 64):                 # windows that reach in front of key 0: no shift, head tiles 0 .. 2
            for c in (-60, -5, 0, 40, 200):
                if lk + c >= 1:
                    yield (lk + c, lq, lk)


PACKED_BR_WANTED = {("form", 0, r) for r in RUNS} | {("loop", t, r) for t, r in TRIPS_REM} | {("diag", d, True) for d in (False, True)}
PACKED_WINDOW_WANTED = {("form", nh, r) for nh in range(4) for r in RUNS} | {("loop", t, r) for t, r in TRIPS_REM} | \
    {("diag", d, True) for d in (False, True)}
# rows in front of key 0, a lone key, no keys, no rows
PACKED_SPECIAL = ((300, 130), (7, 1), (64, 0), (0, 200))


@functools.lru_cache(maxsize=None)
def packed_br_pairs():
    return tuple((lq, lk) for _, lq, lk in _greedy(_packed_br_candidates(), _packed_keys, PACKED_BR_WANTED)) + PACKED_SPECIAL


@functools.lru_cache(maxsize=None)
def packed_window_cases():
    """((W, ((Lq_b, Lk_b), ...)), ...): the window is one per call, so the selection is grouped by it."""
    picked = _greedy(_packed_window_candidates(), _packed_keys, PACKED_WINDOW_WANTED)
    groups = collections.OrderedDict()
    for W, lq, lk in picked:
        groups.setdefault(W, []).append((lq, lk))
    first = next(iter(groups))
    groups[first] += list(PACKED_SPECIAL)
    return tuple((W, tuple(pairs)) for W, pairs in groups.items())


def packed_plans(W: int, pairs):
    return {(lq, lk, j): packed(lq, lk, W, j) for lq, lk in pairs for j in range(nblk(lq))}


# ---- (f) num_splits: the chunks of the kv_lens split (tests/test_gpu_split_tile_counts.py).  Keys padded to 2560 (40 tiles); with S = 2 a chunk
# holds T = 20 tiles, so a chunk's pipelined run reaches 18: two trips and every remainder.  One query block; the unpacked form at Lq in {1, 33,
# 128}, the packed one at Lq in {1, 16, 32}.
LKP_SPLIT, S_SPLIT = 2560, 2
SPLIT_UNPACKED_LQS = (1, 33, 128)
SPLIT_LQS = tuple(sorted(set(PACK_LQS + SPLIT_UNPACKED_LQS)))
# non-causal: chunk 0 (no chunk in front of it) and chunk 1 (seeded behind a full chunk 0) as a partial chunk of every whole-tile count 0 .. 20,
# with a whole last tile and with tails of 1 and 63 keys; chunk 1 empty; no keys; everything
SPLIT_LENS = tuple(sorted({0, LKP_SPLIT} | {c + 64 * t + e for c in (0, 1280) for t in range(21) for e in (0, 1, 63) if c + 64 * t + e <= LKP_SPLIT}))


def split_plans(causal: bool, lq: int, cases, Lkp: int = LKP_SPLIT, S: int = S_SPLIT):
    """{(len, s, chunk): Plan} of ``cases``: lengths (non-causal; s None) or (len, s) pairs (causal)."""
    cases = [(n, None) for n in cases] if not causal else list(cases)
    return {(n, s, c): split_chunk(causal, lq, Lkp, n, s, S, c) for n, s in cases for c in range(S)}


def _split_keys(causal, case, Lkp=LKP_SPLIT, S=S_SPLIT, lqs=SPLIT_LQS):
    """What a case reaches, per Lq and chunk: the pipelined loop's partition and the last-tile bodies of every non-empty chunk; the chunks
    without work by their cause."""
    n, s = case if causal else (case, None)
    keys = set()
    for lq in lqs:
        for c in range(S):
            p = split_chunk(causal, lq, Lkp, n, s, S, c)
            if p.lk == 0:
                if min(max(n, 0), Lkp) > 0:
                    keys.add((lq, "past_len"))             # a chunk from len_b on, of a sample that has keys
                continue
            if p.n_iters == 0:
                keys.add((lq, "behind_diagonal"))
                continue
            keys.add((lq, "loop", c, p.trips, p.remainder))
            if causal:                                     # the run in front of the pipelined diagonal bodies and in front of general tiles
                keys.add((lq, "diagonal", c, p.trips, p.remainder, p.diag_ok))
            keys.add((lq, "last", p.diag_ok if causal else p.tail_ok, p.run > 0))
            if p.lk < BLKK:
                keys.add((lq, "one_ragged_tile"))
    return keys


def _split_wanted(causal):
    per_lq = {("loop", c, t, r) for c in range(S_SPLIT) for t, r in TRIPS_REM} | {("last", True, True), ("last", True, False)} | \
        {("past_len",), ("one_ragged_tile",)}
    if causal:
        per_lq |= {("behind_diagonal",), ("last", False, True)} | {("diagonal", c, t, r, d) for c in range(S_SPLIT) for t, r in TRIPS_REM for d in (False, True)}
    return {(lq,) + k for lq in SPLIT_LQS for k in per_lq}


# causal: (len, s).  Offset 64 k + e puts k steady tiles of the chunk it falls into in front of the diagonal; e = 0 keeps the pipelined diagonal
# bodies, any other e puts the diagonal across general tiles.
_SPLIT_GRID_LENS = (LKP_SPLIT, 2497, 1281, 1280, 1279, 1217, 700, 65)
_SPLIT_EDGE = LKP_SPLIT // S_SPLIT            # the first key of chunk 1


def _split_causal_candidates():
    for k in range(-2, 41):
        for e in (0,) + tuple((1, 37, 63)[(k + i) % 3] for i in range(3)):      # (the first of equals is taken: rotate the unaligned ones)
            for n in _SPLIT_GRID_LENS:
                yield (n, 64 * k + e)
    for n in SPLIT_LENS:                      # bottom-right: the last row's diagonal on the last key
        for lq in SPLIT_LQS:
            yield (n, n - lq)


# the diagonal of row 0 / of the last row exactly on the chunk boundary and one key to either side; bottom-right at every Lq; rows in front of key 0; offsets at and behind
# the length; a sample without keys
SPLIT_CAUSAL_SPECIAL = tuple((n, _SPLIT_EDGE - r + d) for n in (LKP_SPLIT, 1300) for r in (0, 127, 32) for d in (-1, 0, 1)) + \
    tuple((n, n - lq) for n in (LKP_SPLIT, 1343, 1281) for lq in SPLIT_LQS) + ((LKP_SPLIT, -1), (1500, -64), (LKP_SPLIT, -130), (700, 700), (700, 900), (1300, 1300), (1300, LKP_SPLIT), (0, 5), (0, 0))


@functools.lru_cache(maxsize=None)
def split_causal_pairs():
    picked = _greedy(_split_causal_candidates(), functools.partial(_split_keys, True), _split_wanted(True))
    return picked + tuple(p for p in SPLIT_CAUSAL_SPECIAL if p not in picked)


# chunk counts: (padded length, S, lengths of the non-causal call, (len, s) pairs of the causal one) -- one tile per chunk; two; four with
# trailing chunks past the tensor; the full width of the 8-bit count (215 chunks past the tensor, the longest seed prefix); a padded length that is
# no multiple of 64 (41 tiles, the last of one key).  Full and ragged lengths, bottom-right at Lq 33 and unaligned offsets.
def _count_entry(Lkp, S):
    return (Lkp, S, (Lkp, Lkp - 27, 1345, 0), ((Lkp, Lkp - 33), (Lkp - 27, Lkp - 27 - 33), (Lkp, 1061), (1345, 1280), (Lkp - 27, -5)))


SPLIT_COUNT_CASES = tuple(_count_entry(Lkp, S) for Lkp, S in ((2560, 40), (2560, 20), (2560, 13), (2560, 255), (2561, 3)))


# ================================================================================================ the seeded random sweep of the keyword family
RANDOM_LKS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 256, 320, 449, 512, 576, 640, 705, 832, 1000, 1024, 1216, 1536)


def random_call(seed: int) -> dict:
    """One call of the dense FP8-PV entry point with its keyword family drawn from ``seed`` (tests/test_gpu_route_random.py): shapes, per-sample
    lengths, one kind of offset, one kind of window, ``pack_gqa`` where the route takes it.  Pure Python, so that the host test can judge the
    generator without a GPU."""
    import random
    rng = random.Random(31000 + seed)
    c = dict(seed=seed, D=rng.choice((64, 128, 96)), dtype=rng.choice(("f16", "bf16")), layout=rng.choice(("HND", "NHD")), smooth_k=rng.random() < 0.5,
             B=rng.randint(1, 3), Hkv=rng.randint(1, 2), group=rng.choice((1, 2, 4)))
    c["Lq"] = Lq = rng.randint(1, 32) if rng.random() < 0.5 else rng.randint(33, 420)
    # (mostly at least as many keys as rows: with far fewer, most rows of most offsets and windows stand behind the last key)
    c["Lk"] = Lk = rng.choice([n for n in RANDOM_LKS if n >= Lq] if rng.random() < 0.93 else RANDOM_LKS)
    # lengths: anywhere in [0, Lk], but mostly long enough for the rows to see keys (a uniform draw leaves most offsets behind the keys)
    c["lens"] = [rng.choice((Lk, rng.randint(0, Lk), rng.randint(max(0, Lk - 70), Lk), rng.randint(Lk // 2, Lk))) for _ in range(c["B"])]
    window = rng.choice(("none", "causal", "two_sided"))
    offset = rng.choice(("none", "bottom_right", "int", "tensor"))
    left = rng.choice((0, 1, 63, 64, 100, rng.randint(0, Lk + Lq)))
    c["window_size"] = None if window == "none" else (left, 0) if window == "causal" else (left, rng.choice((0, 1, 30, rng.randint(0, 200))))
    c["is_causal"] = True if (window == "causal" or (window == "none" and offset != "none")) else False if window == "two_sided" else rng.random() < 0.5
    c["causal_align"], c["q_start"] = "top_left", None
    near = lambda n: rng.choice((n - Lq, n - Lq, 0, rng.randint(-Lq - 5, Lk + 5), rng.randint(max(-Lq - 5, n - Lq - 64), min(Lk + 5, n - Lq + 64))))
    if offset == "bottom_right":
        c["causal_align"] = "bottom_right"
    elif offset == "int":
        c["q_start"] = near(min(c["lens"]))
    elif offset == "tensor":
        c["q_start"] = [near(n) for n in c["lens"]]
    c["pack_gqa"] = bool(Lq <= 32 and c["group"] >= 2 and rng.random() < 0.7)
    return c


def random_call_geometry(c: dict):
    """Per sample ``(length, offset s_b of the diagonal, window_size for the predicate, is_causal for the predicate)``: what
    ``ref_window.visible_from_keywords`` takes."""
    out = []
    for b, n in enumerate(c["lens"]):
        if c["causal_align"] == "bottom_right":
            s = n - c["Lq"]
        elif c["q_start"] is None:
            s = 0
        else:
            s = c["q_start"] if isinstance(c["q_start"], int) else c["q_start"][b]
        ws = c["window_size"]
        if ws is None:
            ws = (-1, 0) if c["is_causal"] else (-1, -1)
        out.append((n, s, ws, c["is_causal"]))
    return out


# ================================================================================================ the seeded random sweep of num_splits
SPLIT_RANDOM_LKS = RANDOM_LKS + (2049, 2560)
SPLIT_RANDOM_S = ("2", "3", "4", "7", "tiles", "tiles+3", "255")
SPLIT_RANDOM_OFFSETS = ("none", "top_left", "bottom_right", "int", "tensor")


def random_split_call(seed: int) -> dict:
    """One ``num_splits=`` call of the dense FP8-PV entry point drawn from ``seed`` (tests/test_gpu_split_random.py), with a stream of its own:
    ``random_call`` draws what it drew before this generator existed.  One query block (Lq <= 128), no window that bounds the look-back (the
    keyword refuses both); the keys of the dictionary are ``random_call``'s, plus ``S`` (the chunk count: at least 2, 1 being the call without
    the keyword) and the names of what was drawn (``S_kind``, ``offset``)."""
    import random
    rng = random.Random(47000 + seed)
    c = dict(seed=seed, D=rng.choice((64, 128, 96)), dtype=rng.choice(("f16", "bf16")), layout=rng.choice(("HND", "NHD")), smooth_k=rng.random() < 0.5,
             B=rng.randint(1, 3), Hkv=rng.randint(1, 2), group=rng.choice((1, 2, 4, 5)))
    c["Lq"] = Lq = rng.randint(1, 32) if rng.random() < 0.5 else rng.randint(33, 128)
    c["Lk"] = Lk = rng.choice([n for n in SPLIT_RANDOM_LKS if n >= Lq] if rng.random() < 0.93 else SPLIT_RANDOM_LKS)
    c["lens"] = [rng.choice((Lk, rng.randint(0, Lk), rng.randint(max(0, Lk - 70), Lk), rng.randint(Lk // 2, Lk))) for _ in range(c["B"])]
    c["offset"] = offset = rng.choice(SPLIT_RANDOM_OFFSETS)
    c["window_size"], c["is_causal"], c["causal_align"], c["q_start"] = None, offset != "none", "top_left", None
    near = lambda n: rng.choice((n - Lq, n - Lq, 0, rng.randint(-Lq - 5, Lk + 5), rng.randint(max(-Lq - 5, n - Lq - 64), min(Lk + 5, n - Lq + 64))))
    if offset == "bottom_right":
        c["causal_align"] = "bottom_right"
    elif offset == "int":
        c["q_start"] = near(min(c["lens"]))
    elif offset == "tensor":
        c["q_start"] = [near(n) for n in c["lens"]]
    tiles = (Lk + BLKK - 1) // BLKK
    c["S_kind"] = kind = rng.choice(SPLIT_RANDOM_S)
    c["S"] = max(2, {"tiles": tiles, "tiles+3": tiles + 3}.get(kind) or int(kind))
    c["pack_gqa"] = bool(Lq <= 32 and c["group"] >= 2 and rng.random() < 0.7)
    return c


# ================================================================================================ the paged units (tests/test_gpu_paged_tile_counts.py)
# The six paged compilation units -- f8p (the kv_lens / q_start / window forms behind a block table), f8pg (pack_gqa), f8pks (pass 2 of the
# split), f8pr (packed query rows), f8pb / f8pbg (the step call's chunk and decode launches) -- each compile the six-body loop on their own.  A
# paged launch is a KVLEN-family launch whose padded length is the LOGICAL capacity, so ``dense`` / ``split_chunk`` model it as they stand; a
# sequence of the ragged and step calls is the causal item of its own row count.
#
# ONE cache serves every unsplit route: sample b holds PAGED_SAMPLES[b][0] keys, and every causal call places its row 0 at PAGED_SAMPLES[b][1]
# (the lengths of sweep (a) bottom-right at Lq 200, then sweep (b)'s pairs).  A route is a list of calls on that cache; a windowed call has one
# W for all samples, so the windows are chosen greedily by what ALL samples reach under them.
PAGED_PAGE_SIZES = (64, 256)              # a page boundary behind every tile, and behind every fourth
PAGED_HKV, PAGED_GROUPS = 2, (1, 4, 5)
PAGED_RUNS = tuple(range(18))             # 24 tiles: the pipelined run reaches 17 behind a 128-row block's diagonal
PAGED_SAMPLES = tuple((n, n - LQ) for n in KV_LENS) + Q_START_ALIGNED + Q_START_PAIRS
PAGED_RAGGED_LQS = (1, 32, 33, 128, 130)  # the decode band and its edge, the chunk band's first count, a whole block, two blocks
PAGED_ROTATIONS = len(PAGED_RAGGED_LQS)   # call c of the ragged / step sweep gives sample b PAGED_RAGGED_LQS[(b + c) % 5] rows


def paged_plans(lq: int, causal: bool, W: int = 0):
    """{(sample, query block): Plan} of one dense call on the shared cache (f8p; with lq <= 32 also f8pg)."""
    return {(b, j): dense(128, causal, lq, LKP, n, s if causal else None, W, j) for b, (n, s) in enumerate(PAGED_SAMPLES) for j in range(nblk(lq))}


def _paged_window_keys(W):
    keys = set()
    for (b, j), p in paged_plans(LQ, True, W).items():
        if p.n_iters:
            keys.add(("form", p.nh, p.run))
    for lq in PACK_LQS:
        for p in paged_plans(lq, True, W).values():
            if p.n_iters and p.nh > 0:
                keys.add(("pack", lq, p.run))
    return keys


PAGED_WINDOW_WANTED = {("form", nh, r) for nh in range(4) for r in RUNS} | {("pack", lq, r) for lq in PACK_LQS for r in RUNS}


@functools.lru_cache(maxsize=None)
def paged_windows():
    """The W of the windowed calls: each is one call per route on every sample."""
    return _greedy([64 * m + d for m in range(0, 24) for d in (0, 1, 37, 63) if 64 * m + d >= 1], _paged_window_keys, PAGED_WINDOW_WANTED)


def paged_ragged_counts(rotation: int):
    return tuple(PAGED_RAGGED_LQS[(b + rotation) % PAGED_ROTATIONS] for b in range(len(PAGED_SAMPLES)))


def paged_ragged_plans(rotation: int, W: int = 0, bottom_right: bool = False):
    """{(sample, query block): (band, Plan)} of one ragged / step call: ``band`` names the launch and the block -- "decode" (1 .. 32 rows: the step
    call's packed-group launch), "chunk" (one block of 33 .. 128 rows), "two0" / "two1" (the blocks of a 130-row sequence).  The offsets are the
    samples' own (clamped to -Lq_b, which moves no row that sees a key), or with ``bottom_right`` len_b - Lq_b."""
    out = {}
    for b, ((n, s), lq) in enumerate(zip(PAGED_SAMPLES, paged_ragged_counts(rotation))):
        s = n - lq if bottom_right else max(s, -lq)
        for j in range(nblk(lq)):
            band = "decode" if lq <= 32 else "chunk" if lq <= BLKQ else f"two{j}"
            out[(b, j)] = (band, dense(128, True, lq, LKP, n, s, W, j))
    return out


PAGED_BANDS = ("decode", "chunk", "two0", "two1")

# ---- f8pks: a cache of its own, capacity 2560 as sweep (f), so that a chunk of S = 2 holds 20 tiles.  S 3: T = 14 -- with pages of 256 keys chunk
# 1 starts at tile 2 of page 3 and chunk 2 reaches past the table; S 5: T = 8.  The samples: sweep (f)'s non-causal lengths (bottom-right at the
# widest block for the causal calls) and its causal pairs.
PAGED_SPLITS = (2, 3, 5)
PAGED_SPLIT_LQS = (1, 16, 128)            # packed at 1 and 16 (the groups of 4 and 5), unpacked at 16 and 128


@functools.lru_cache(maxsize=None)
def paged_split_samples():
    return tuple((n, n - BLKQ) for n in SPLIT_LENS) + split_causal_pairs()


def paged_split_plans(causal: bool, lq: int, S: int):
    return {(b, c): split_chunk(causal, lq, LKP_SPLIT, n, s if causal else None, S, c) for b, (n, s) in enumerate(paged_split_samples()) for c in range(S)}


def paged_anchor(plans, key=lambda kk: kk[1] == 0):
    """(sample, Plan) of the first work item of ``plans`` -- {(sample, block or chunk): Plan or (band, Plan)}, those ``key`` admits -- that runs at
    least two trips of the six-body loop and a remainder: the sample a sweep holds to the attention reference."""
    for kk, p in plans.items():
        p = p if isinstance(p, Plan) else p[1]
        if key(kk) and p.n_iters and p.trips >= 2 and p.remainder > 0:
            return kk[0], p
    raise AssertionError("no work item with two trips and a remainder")


@functools.lru_cache(maxsize=None)
def paged_ragged_anchor(band: str):
    """(rotation, sample, Plan): the first call of the ragged / step sweep, without a window, that has such a work item in ``band``."""
    for r in range(PAGED_ROTATIONS):
        plans = paged_ragged_plans(r)
        try:
            return (r,) + paged_anchor(plans, key=lambda kk: plans[kk][0] == band)
        except AssertionError:
            continue
    raise AssertionError(band)


@functools.lru_cache(maxsize=None)
def paged_window_anchor():
    """(W, sample, Plan): the first windowed call of the dense sweep with such a work item behind head tiles, in either query block."""
    for W in paged_windows():
        plans = paged_plans(LQ, True, W)
        try:
            return (W,) + paged_anchor(plans, key=lambda kk: plans[kk].nh > 0)
        except AssertionError:
            continue
    raise AssertionError("no window")
