"""GPU: tile-count sweep of pass 2 of the kv_lens split (``num_splits=``: the ``*_f8ks`` units, SEED with KVLEN) and of its length-aware pass 1.

Each ``f8ks`` unit compiles its own copy of the hand-scheduled pipelined loop (csrc/sage_attn_loop_f8.h), and a chunk's loop partition is that
of a call on the chunk's keys.  tests/test_gpu_kv_split.py runs the units at 17 tiles, where a chunk holds 9, 5, 2 or 1: a pipelined run of 7
at the most, never a second trip, no remainder behind a trip.  Here the keys are padded to 2560 (40 tiles) and split in two (T = 20), and the
lengths and offsets are CHOSEN with ``loop_plan.split_chunk`` -- the host model of a chunk's partition -- so that chunk 0 (no chunk in front of
it) and chunk 1 (seeded behind a full chunk 0) each run 0, 1 and 2 trips with every remainder 0 .. 5, with and without the last-tile bodies, in
front of the pipelined diagonal bodies and in front of general tiles; chunks past len_b, behind the diagonal and of one ragged tile are among
them.  A third table walks the chunk counts: T = 1 (S = 40), 2 (S = 20), 4 with trailing chunks past the tensor (S = 13), the full width of the
8-bit count (S = 255: 215 chunks past the tensor, the longest seed prefix) and a padded length that is no multiple of 64 (2561, S = 3).  What the
tables reach is asserted in tests/test_loop_plan_host.py on the CPU, next to the check of the model; every case prints the model's forms per
chunk next to its distances.

References, both the project's own, neither loosened:
  a. every case against the same call without ``num_splits`` at test_gpu_kv_split.py::_distance's bars for "summation order only" (2 output
     ulps + 1e-5 max|o| per element, rel-RMS 1e-3, LSE 1e-5 relative, -inf matching -inf); rows without a visible key exactly +0 / -inf; the
     packed split equals the unpacked split bit for bit; the grid probe confirms pass 2's grid on every call (B Hq S unpacked, B Hkv
     ceil(group / 4) S packed); the non-causal table once more with the caller's rows from len_b on overwritten (0xFF, 0x5A): the same bits;
  b. the causal table and the chunk-count table against ``ref_window.attn_window`` under ``visible(Lq, n, s, 0, 0, n)`` on the oracle's
     quantised operands (test_gpu_route_tile_counts.py::check_sample: 2e-3 max|ref| + 2 output ulps, LSE within 5e-3), eight samples per test.

Shapes: Hkv = 1, D in {128, 64}, the dtype alternating with the case, K with a per-channel bias, padding rows random data.  Unpacked: Hq = 2, Lq
in {1, 33, 128}; packed: groups of 4 (four heads in one workgroup) and 5 (a second workgroup with three idle waves), Lq in {1, 16, 32}.  One
call per table carries all its samples in the batch.

Reference cost of (b), measured on the CPU at these shapes (each test prints it): 0.007 - 0.029 s per sample of up to 2560 keys at Lq 1, 33
and 128 -- 0.06 - 0.23 s per chunk of eight causal samples, 0.17 - 0.19 s for the nine samples of a chunk-count entry; (a) compares GPU
results only.
"""
import ctypes
import functools
import time

import pytest
import torch

import loop_plan as lp
import ref_window as rw
from test_gpu_kv_split import _distance, _poisoned
from test_gpu_route_tile_counts import check_sample

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, ops
    DEV = torch.device("cuda:0")

HKV, LKP, S2 = 1, lp.LKP_SPLIT, lp.S_SPLIT
F16, BF16 = torch.float16, torch.bfloat16
DS = (128, 64)
NB = 128                                  # samples of the widest table's call
FILLS = (0xFF, 0x5A)
FP8 = lambda *a, **kw: sa.sageattn_qk_int8_pv_fp8_cuda(*a, **kw)
# (packed?, Lq, Hq)
FORMS = [(False, lq, 2) for lq in lp.SPLIT_UNPACKED_LQS] + [(True, lq, g) for lq in lp.PACK_LQS for g in lp.PACK_GROUPS]
FORM_IDS = [f"{'pk' if pk else 'un'}-lq{lq}-h{hq}" for pk, lq, hq in FORMS]
TABLES = {"nc": tuple((n, None) for n in lp.SPLIT_LENS), "causal": lp.split_causal_pairs()}
assert max(len(t) for t in TABLES.values()) <= NB


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()
    yield
    _kv.cache_clear()                     # (the tables' K / V and Q: about 0.5 GB of device memory, this module's alone)
    _q.cache_clear()


def _ints(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _kv(D, dt, Lkp=LKP, nb=NB):
    """k / v [nb, 1, Lkp, D] (HND, K with a per-channel bias) on the device: made once per shape, never modified, released behind the module's
    last test (the ``_gpu`` fixture)."""
    g = torch.Generator().manual_seed(41 + D + Lkp)
    k = (torch.randn(nb, HKV, Lkp, D, generator=g) + torch.randn(1, HKV, 1, D, generator=g)).to(dt)
    v = torch.randn(nb, HKV, Lkp, D, generator=g).to(dt)
    return k.to(DEV), v.to(DEV)


@functools.lru_cache(maxsize=None)
def _q(D, dt, hq, lq, nb=NB):
    g = torch.Generator().manual_seed(43 + D + 7 * hq + lq)
    return torch.randn(nb, hq, lq, D, generator=g).to(dt).to(DEV)


def _keywords(cases):
    """The keywords of a table's call: lengths, and offsets where the table is causal."""
    causal = cases[0][1] is not None
    kw = dict(is_causal=causal, kv_lens=_ints([n for n, _ in cases]))
    if causal:
        kw["q_start"] = _ints([s for _, s in cases])
    return causal, kw


def _call(q, k, v, kw, S, packed, probe):
    """One call; with ``S`` the grid probe must report pass 2's grid, without it the unsplit launch's."""
    nb, hq = q.shape[0], q.shape[1]
    probe.value = -1
    with ops.launch_hooks(grid_probe=probe):
        out = FP8(q, k, v, return_lse=True, pack_gqa=packed, num_splits=S, **kw)
    torch.cuda.synchronize()
    wgs = nb * HKV * ((hq // HKV + 3) // 4) if packed else nb * hq
    assert probe.value == wgs * (S or 1), (probe.value, nb, hq, S, packed)
    return out


def _rows_without_keys(causal, lq, n, s, Lkp):
    """How many leading rows of a sample see no key: all without keys, else (causal) the rows in front of key 0."""
    if min(max(n, 0), Lkp) < 1:
        return lq
    return min(lq, max(0, -s)) if causal else 0


def _describe(causal, lq, n, s, Lkp, S):
    """The model's forms of the chunks that run, and how many chunks do not."""
    plans = [lp.split_chunk(causal, lq, Lkp, n, s, S, c) for c in range(S)]
    run = [f"c{c}[{p.lk}]{lp.describe(p)}" for c, p in enumerate(plans) if p.lk > 0 and p.n_iters > 0]
    past = sum(1 for p in plans if p.lk == 0)
    behind = sum(1 for p in plans if p.lk > 0 and p.n_iters == 0)
    return " ".join(run) + f" | {past} chunks past len, {behind} behind the diagonal"


def _check_against_unsplit(tag, cases, got, want, dt, lq, Lkp, S):
    """(a): the call at the bars of "summation order only"; every sample's own distances printed next to the model's forms; rows without a
    visible key exactly +0 / -inf."""
    causal = cases[0][1] is not None
    for b, (n, s) in enumerate(cases):
        e, r, l = _distance((got[0][b:b + 1], got[1][b:b + 1]), (want[0][b:b + 1], want[1][b:b + 1]), dt)
        print(f"{tag} len {n} offset {s}: element {e:.3f} rel-RMS {r:.3f} lse {l:.3f} of their bars; {_describe(causal, lq, n, s, Lkp, S)}")
        none = _rows_without_keys(causal, lq, n, s, Lkp)
        assert bool(torch.isneginf(got[1][b, :, :none]).all()) and bool(torch.isfinite(got[1][b, :, none:]).all()), (tag, n, s)
        ob = got[0][b, :, :none].float()
        assert not bool(ob.any()) and not bool(torch.signbit(ob).any()), (tag, n, s)          # +0, not merely small
    elem, rms, lse = _distance(got, want, dt)
    print(f"WORST {tag}: element {elem:.3f} rel-RMS {rms:.3f} lse {lse:.3f} of their bars")
    assert elem <= 1.0 and rms <= 1.0 and lse <= 1.0, (tag, elem, rms, lse)


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: o differs in {int((a[0] != b[0]).sum())} of {a[0].numel()} elements"
    assert torch.equal(a[1], b[1]), f"{what}: lse differs in {int((a[1] != b[1]).sum())} of {a[1].numel()} rows"


# ---------------------------------------------------------------------------------------------- a. against the call without num_splits
@pytest.mark.parametrize("form", range(len(FORMS)), ids=FORM_IDS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("table", list(TABLES))
def test_tables_match_the_unsplit_call(table, D, form):
    packed, lq, hq = FORMS[form]
    cases = TABLES[table]
    nb = len(cases)
    dt, smooth_k = (F16, BF16)[(form + DS.index(D) + (table == "causal")) & 1], bool(form & 2)
    k, v = (t[:nb] for t in _kv(D, dt))
    q = _q(D, dt, hq, lq)[:nb]
    causal, kw = _keywords(cases)
    kw["smooth_k"] = smooth_k
    probe = ctypes.c_int32(-1)
    got = _call(q, k, v, kw, S2, packed, probe)
    want = _call(q, k, v, kw, None, packed, probe)
    tag = f"{table} d{D} {FORM_IDS[form]}"
    _check_against_unsplit(tag, cases, got, want, dt, lq, LKP, S2)
    if packed:
        _same(got, _call(q, k, v, kw, S2, False, probe), f"{tag}: the packed split against the unpacked split")


COUNT_FORMS = ((False, 33, 2), (True, 16, 5), (False, 128, 2), (True, 1, 4))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("entry", range(len(lp.SPLIT_COUNT_CASES)), ids=[f"lk{e[0]}-s{e[1]}" for e in lp.SPLIT_COUNT_CASES])
def test_chunk_counts_match_the_unsplit_call(entry, D):
    Lkp, S, lens, pairs = lp.SPLIT_COUNT_CASES[entry]
    probe = ctypes.c_int32(-1)
    for i, (packed, lq, hq) in enumerate(COUNT_FORMS):
        dt = (F16, BF16)[(entry + i + DS.index(D)) & 1]
        for cases in (tuple((n, None) for n in lens), pairs):
            nb = len(cases)
            k, v = (t[:nb] for t in _kv(D, dt, Lkp, 8))
            q = _q(D, dt, hq, lq, 8)[:nb]
            causal, kw = _keywords(cases)
            kw["smooth_k"] = bool(i & 1)
            got = _call(q, k, v, kw, S, packed, probe)
            want = _call(q, k, v, kw, None, packed, probe)
            tag = f"counts lk{Lkp} s{S} {'causal' if causal else 'nc'} d{D} {'pk' if packed else 'un'}-lq{lq}-h{hq}"
            _check_against_unsplit(tag, cases, got, want, dt, lq, Lkp, S)
            if packed:
                _same(got, _call(q, k, v, kw, S, False, probe), f"{tag}: the packed split against the unpacked split")


# ---------------------------------------------------------------------------------------------- a. padding
PAD_FORMS = (1, 2, 5, 6)                  # unpacked Lq 33 and 128, packed Lq 16 group 4 and 5


@pytest.mark.parametrize("form", PAD_FORMS, ids=[FORM_IDS[i] for i in PAD_FORMS])
@pytest.mark.parametrize("D", DS)
def test_rows_behind_the_lengths_are_never_read(D, form):
    """The non-causal table with the caller's rows from len_b on overwritten with 0xFF (NaN) and with 0x5A: the clean run's bits."""
    packed, lq, hq = FORMS[form]
    cases = TABLES["nc"]
    nb = len(cases)
    dt = (F16, BF16)[(form + DS.index(D)) & 1]
    k, v = (t[:nb] for t in _kv(D, dt))
    q = _q(D, dt, hq, lq)[:nb]
    causal, kw = _keywords(cases)
    probe = ctypes.c_int32(-1)
    want = _call(q, k, v, kw, S2, packed, probe)
    lens = [n for n, _ in cases]
    for fill in FILLS:
        got = _call(q, _poisoned(k, lens, "HND", fill), _poisoned(v, lens, "HND", fill), kw, S2, packed, probe)
        _same(got, want, f"d{D} {FORM_IDS[form]} padding byte 0x{fill:02X}")


# ---------------------------------------------------------------------------------------------- b. against the restatement
def _chunks(seq, n):
    return [tuple(seq[i:i + n]) for i in range(0, len(seq), n)]


CAUSAL_CHUNKS = _chunks(TABLES["causal"], 8)
RESTATED_LQS = (128, 33, 1)


def _check_restated(oracle, tag, cases, q, k, v, got, code, D, smooth_k, lq, Lkp, S):
    causal = cases[0][1] is not None
    t0 = time.perf_counter()
    for b, (n, s) in enumerate(cases):
        nv = max(0, min(n, Lkp))
        keep = rw.visible(lq, nv, s if causal else nv, 0, 0, nv)          # (non-causal: every row's diagonal behind the last key)
        check_sample(oracle, f"{tag} len {n} offset {s} {_describe(causal, lq, n, s, Lkp, S)}", q[b:b + 1], k[b:b + 1, :, :nv].contiguous(),
                     v[b:b + 1, :, :nv].contiguous(), code, D, smooth_k, keep, got[0][b:b + 1], got[1][b:b + 1])
    print(f"RESTATEMENT {tag}: {(time.perf_counter() - t0) / len(cases):.3f} s per sample (Lq {lq}, {len(cases)} samples)")


@pytest.mark.parametrize("chunk", range(len(CAUSAL_CHUNKS)))
def test_causal_table_vs_restatement(oracle_mod, chunk):
    cases = CAUSAL_CHUNKS[chunk]
    D, lq = DS[chunk & 1], RESTATED_LQS[chunk % 3]
    dt, smooth_k = (F16, BF16)[(chunk >> 1) & 1], bool(chunk & 4)
    code = 0 if dt == F16 else 1
    nb = len(cases)
    k, v = (t[:nb] for t in _kv(D, dt))
    q = _q(D, dt, 2, lq)[:nb]
    causal, kw = _keywords(cases)
    kw["smooth_k"] = smooth_k
    got = _call(q, k, v, kw, S2, False, ctypes.c_int32(-1))
    _check_restated(oracle_mod, f"causal d{D}", cases, q, k, v, got, code, D, smooth_k, lq, LKP, S2)


@pytest.mark.parametrize("entry", range(len(lp.SPLIT_COUNT_CASES)), ids=[f"lk{e[0]}-s{e[1]}" for e in lp.SPLIT_COUNT_CASES])
def test_chunk_counts_vs_restatement(oracle_mod, entry):
    """Lq = 33, where the table's bottom-right pairs put the last row's diagonal on the last key; the non-causal lengths and the causal pairs of
    an entry are nine samples, one of them without keys."""
    Lkp, S, lens, pairs = lp.SPLIT_COUNT_CASES[entry]
    D, lq = DS[entry & 1], 33
    dt, smooth_k = (F16, BF16)[(entry >> 1) & 1], bool(entry & 1)
    code = 0 if dt == F16 else 1
    for cases in (tuple((n, None) for n in lens), pairs):
        nb = len(cases)
        k, v = (t[:nb] for t in _kv(D, dt, Lkp, 8))
        q = _q(D, dt, 2, lq, 8)[:nb]
        causal, kw = _keywords(cases)
        kw["smooth_k"] = smooth_k
        got = _call(q, k, v, kw, S, False, ctypes.c_int32(-1))
        _check_restated(oracle_mod, f"counts lk{Lkp} s{S} d{D}", cases, q, k, v, got, code, D, smooth_k, lq, Lkp, S)
