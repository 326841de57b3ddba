"""GPU: one attention call per engine step on the paged quantised KV cache (``sageattention_amd.paged_kv_step``, ``sage_kvstep_attn``;
DESIGN 3.22).

``sageattn_kvcache_step`` sorts the sequences of a packed batch on the device -- 1 .. 32 rows: the packed-group kernel, four query heads of a GQA
group per workgroup; more: the 128-row kernel -- and returns what ``sageattn_kvcache_varlen`` returns.  The reference is that route, the bar is
bit equality, no tolerance:
  A  ``o`` and ``lse`` (smoothed cache, K-mean correction included) equal the ragged route's bits on every row, and every row no sequence owns --
     the slack behind ``total``, the rows of a sequence beyond ``max_seqlen_q`` -- keeps the poison of the pre-poisoned outputs; both bands, an
     idle slot, two query blocks, the band's edge on both sides (32 / 33 rows), one-launch steps, a sequence cut to 32 rows, an explicit
     ``q_start``, a decode sequence of ten tiles;
  B  ``grid_out`` is ``B * Hkv * ceil(group / 4)`` when ``max_seqlen_q <= 32`` and that plus ``B * Hq * ceil(max_seqlen_q / 128)`` otherwise: the
     decode rows are packed;
  C  in guarded, poisoned memory a well-formed call and calls with non-monotone, negative, past-``total`` and mixed prefix arrays leave every
     guard untouched (wrong numbers are allowed there; the band's own proof is the host program of tests/test_kv_step_host.py);
  D  append plus the step call captured into a graph with ``max_seqlen_q`` 130: replays with other prefix contents -- one moves a sequence from
     1 row to 40 rows, from one launch's band into the other's -- equal the eager sequence.

Shapes: B 4, Hkv 2, Hq 8 / 12 / 4 (group 4; group 6: two blocks, the second with two idle waves; group 2: two idle waves), D 64 / 128,
fp16 / bf16, pages of 64 and 128 keys in a poisoned pool of 32 pages behind an interleaved, non-ascending table, logical capacity 640.
"""
import ctypes

import pytest
import torch

from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi, ops
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    from sageattention_amd.paged_kv_step import sageattn_kvcache_step
    from sageattention_amd.paged_kv_varlen import append_varlen, sageattn_kvcache_varlen
    DEV = torch.device("cuda:0")

# (the fixtures of the ragged route's tests: the poisoned pool, its table, the shared caches -- built once per (D, dtype, page size, context))
from test_gpu_kv_varlen import B, BF16, CAP, CONTEXTS, F16, HKV, NUM_PAGES, PAGE_SIZES, POISON, PREFIXES, WINDOWS, _bits, _cache, _content, _cu, _ints, _table, _u8

# (Hq, D, dtype): group 4 everywhere, groups 6 and 2 at one head size and dtype each
CASES = [(8, 64, F16), (8, 64, BF16), (8, 128, F16), (8, 128, BF16), (12, 128, BF16), (12, 64, F16), (4, 128, BF16), (4, 64, F16)]
CASE_IDS = [f"hq{h}-d{D}-{'f16' if dt == F16 else 'bf16'}" for h, D, dt in CASES]
# (query counts, max_seqlen_q)
QUERIES = [((1, 40, 0, 130), 130),       # both bands, an idle slot, two query blocks
           ((32, 33, 1, 0), 33),         # the band's edge on both sides
           ((5, 32, 16, 1), 32),         # one launch only
           ((1, 1, 1, 1), 1),
           ((40, 1, 3, 0), 32)]          # a sequence cut to 32 rows: its first 32 rows, in the decode launch


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _packed_q(Hq, D, dt, counts, slack=0, seed=11):
    g = torch.Generator().manual_seed(seed + D + Hq + sum(counts))
    return torch.randn(sum(counts) + slack, Hq, D, generator=g).to(dt).to(DEV)


def _owned(counts, max_q, rows):
    """bool [rows]: the packed rows some sequence owns and the call computes."""
    m, cu = torch.zeros(rows, dtype=torch.bool), _cu(counts)
    for b, n in enumerate(counts):
        m[cu[b]:cu[b] + min(n, max_q)] = True
    return m.to(DEV)


def _both(q, cache, cu, max_q, **kw):
    """The step call and the ragged call on the same operands, each into outputs pre-poisoned by the fence: (o, lse) of each."""
    out = []
    for fn in (sageattn_kvcache_step, sageattn_kvcache_varlen):
        with Fence(POISON) as f:                    # (o and lse are the package's torch.empty: poisoned bodies between guards)
            o, lse = fn(q, cache, cu, max_q, return_lse=True, **kw)
            f.check()
            out.append((o.clone(), lse.clone()))
    return out


def _assert_same(q, cache, counts, max_q, what, slack=3, **kw):
    total, cu = sum(counts), _ints(_cu(counts))
    (o, lse), (o_ref, lse_ref) = _both(q, cache, cu, max_q, **kw)
    assert o.shape == q.shape and lse.shape == (q.shape[1], total + slack) and lse.dtype == torch.float32
    own = _owned(counts, max_q, total + slack)
    do, dl = _bits(o) != _bits(o_ref), _bits(lse) != _bits(lse_ref)
    print(f"{what}: o differs in {int(do.sum())} of {do.numel()}, lse in {int(dl.sum())} of {dl.numel()}")
    assert not bool(do[own].any()), f"{what}: o differs from the ragged route's in {int(do[own].sum())} elements of owned rows"
    assert not bool(dl[:, own].any()), f"{what}: lse differs from the ragged route's in {int(dl[:, own].sum())} elements of owned rows"
    # rows no sequence owns keep the poison; lse's buffer is rescaled on the device by both routes alike, so untouched words stay equal
    assert bool((_u8(o[~own]) == POISON).all()), f"{what}: rows of o no sequence owns were written"
    assert not bool(dl[:, ~own].any()), f"{what}: lse of rows no sequence owns was written"
    assert bool(own.any()) and torch.isfinite(o[own].float()).all()


# ---- A: the ragged route's bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_row_is_the_ragged_routes(case):
    Hq, D, dt = case
    for page_size in PAGE_SIZES:
        for ctx in CONTEXTS:
            cache = _cache(D, dt, page_size, ctx)
            assert cache.k_mean is not None            # (smoothed: the returned lse carries each row's own sequence's correction)
            for counts, max_q in QUERIES:
                q = _packed_q(Hq, D, dt, counts, 3)
                for window in WINDOWS:
                    kw = dict(window_size=window) if window is not None else {}
                    _assert_same(q, cache, counts, max_q, f"hq {Hq} d{D} page {page_size} ctx {ctx} q {counts}/{max_q} window {window}", **kw)
    cache = _cache(D, dt, PAGE_SIZES[0], CONTEXTS[0])
    counts, max_q = QUERIES[0]
    q = _packed_q(Hq, D, dt, counts, 3)
    o = sageattn_kvcache_step(q, cache, _ints(_cu(counts)), max_q)           # without lse: the same o
    assert torch.equal(_bits(o[:sum(counts)]), _bits(sageattn_kvcache_varlen(q, cache, _ints(_cu(counts)), max_q)[:sum(counts)]))


def test_an_explicit_q_start_places_the_rows_of_both_bands():
    Hq, D, dt = 8, 128, F16
    cache = _cache(D, dt, 64, CONTEXTS[0])
    counts, start = (1, 40, 20, 130), _ints([200, 3, -7, 0])         # (rows in front of key 0, rows past the last key)
    q = _packed_q(Hq, D, dt, counts, 3)
    for window in WINDOWS:
        _assert_same(q, cache, counts, 130, f"q_start window {window}", q_start=start, window_size=window)
    _assert_same(q, cache, counts, 130, "q_start int", q_start=5)


def test_a_decode_sequence_of_ten_tiles():
    """Capacity 1024: a one-row sequence over 640 keys -- the pipelined loop and its last-tile bodies inside the packed-group item -- beside one
    and two tiles, and chunks over the same, at both head sizes."""
    ctx = (64, 128, 640, 601)
    for (Hq, D, dt), page_size in (((12, 128, BF16), 64), ((8, 64, F16), 128)):
        cache = _cache(D, dt, page_size, ctx, 1024)
        for counts in ((16, 40, 1, 130), (1, 1, 32, 2), (64, 2, 128, 1)):
            q = _packed_q(Hq, D, dt, counts, 3)
            for window in WINDOWS:
                kw = dict(window_size=window) if window is not None else {}
                _assert_same(q, cache, counts, max(counts), f"cap 1024 hq {Hq} d{D} q {counts} window {window}", **kw)


# ---- B: the grid ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq", [8, 12, 4])
def test_grid_out_counts_packed_decode_workgroups(Hq):
    D, dt = 64, F16
    cache = _cache(D, dt, 64, CONTEXTS[0])
    ngb = (Hq // HKV + 3) // 4
    for counts, max_q in QUERIES + [((1, 1, 1, 1), 32), ((1, 1, 1, 1), 33), ((1, 1, 1, 1), 129)]:
        q = _packed_q(Hq, D, dt, counts)
        probe = ctypes.c_int32(-1)
        with ops.launch_hooks(grid_probe=probe):
            sageattn_kvcache_step(q, cache, _ints(_cu(counts)), max_q)
        want = B * HKV * ngb + (B * Hq * ((max_q + 127) // 128) if max_q > 32 else 0)
        assert probe.value == want, (counts, max_q, probe.value, want)
        with ops.launch_hooks(grid_probe=probe):                                      # the ragged route: one workgroup per query head
            sageattn_kvcache_varlen(q, cache, _ints(_cu(counts)), max_q)
        assert probe.value == B * Hq * ((max_q + 127) // 128)


# ---- C: fence ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
@pytest.mark.parametrize("name", list(PREFIXES))
@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=[CASE_IDS[0], CASE_IDS[4]])
def test_no_prefix_array_reaches_outside_the_packed_tensors(case, name, fill):
    """q, o, lse and cu_seqlens in guarded, poisoned memory: whatever the prefix array holds, both launches leave every guard its fill (the
    numbers of a malformed call are whatever they are)."""
    Hq, D, dt = case
    total = 171
    cache = _cache(D, dt, 64, CONTEXTS[0])
    q = _packed_q(Hq, D, dt, (total,))
    with Fence(fill) as f:
        cu = f.input(_ints(PREFIXES[name]))
        qf = f.input(q)
        for max_q in (130, 32):
            for window in WINDOWS:
                o, lse = sageattn_kvcache_step(qf, cache, cu, max_q, window_size=window, return_lse=True)
                assert f.owns(o) and ("sageattn_kvcache_step", (Hq, total), torch.float32) in f.package_allocations()
                f.check()


# ---- D: graph ------------------------------------------------------------------------------------------------------------------------------
def test_append_and_the_step_call_capture_into_a_graph():
    """``append_varlen`` + ``sageattn_kvcache_step`` captured once with ``max_seqlen_q`` 130; replays with other prefix contents written into the
    captured inputs equal the eager sequence: sequence 0 goes from 1 row to 40 rows and back to none, sequence 1 from 2 rows to 33 -- the band
    is decided on the device."""
    Hq, D, dt, page_size = 8, 128, BF16, 64
    k, v = _content(D, dt)
    n0, total, max_rows = (62, 62, 3, 0), 48, 130
    table = _ints([x for row in _table((200, 200, 200, 200), page_size, CAP // page_size) for x in row]).view(B, -1)

    def fresh():
        return PagedQuantizedKVCache.from_prefill(k[:, :, :64], v[:, :, :64], table, NUM_PAGES, page_size, kv_lens=_ints(n0), v_headroom=1.5)

    def step(cache, k_in, v_in, cu_in, q_in, fn=None):
        append_varlen(cache, k_in, v_in, cu_in, max_rows)
        return (fn or sageattn_kvcache_step)(q_in, cache, cu_in, max_rows, return_lse=True)

    steps = []
    for i, counts in enumerate([(1, 2, 0, 40), (40, 1, 3, 4), (0, 33, 15, 0)]):
        g = torch.Generator().manual_seed(60 + i)
        steps.append(((torch.randn(total, HKV, D, generator=g) + 1.0).to(dt).to(DEV), (0.5 * torch.randn(total, HKV, D, generator=g)).to(dt).to(DEV),
                      _ints(_cu(counts)), torch.randn(total, Hq, D, generator=g).to(dt).to(DEV), sum(counts)))
    eager_cache, ragged_cache = fresh(), fresh()
    eager = [tuple(t.clone() for t in step(eager_cache, *s[:4])) for s in steps]
    ragged = [tuple(t.clone() for t in step(ragged_cache, *s[:4], fn=sageattn_kvcache_varlen)) for s in steps]
    for i, s in enumerate(steps):                  # the eager sequence is the ragged route's on the rows a sequence owns
        assert torch.equal(_bits(eager[i][0][:s[4]]), _bits(ragged[i][0][:s[4]])) and torch.equal(_bits(eager[i][1][:, :s[4]]), _bits(ragged[i][1][:, :s[4]]))

    warm, cache = fresh(), fresh()
    k_in, v_in, cu_in, q_in = (t.clone() for t in steps[0][:4])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(warm, k_in, v_in, cu_in, q_in)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o, lse = step(cache, k_in, v_in, cu_in, q_in)
    for i, (ks, vs, cs, qs, n) in enumerate(steps):
        k_in.copy_(ks), v_in.copy_(vs), cu_in.copy_(cs), q_in.copy_(qs)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(o[:n]), _bits(eager[i][0][:n])) and torch.equal(_bits(lse[:, :n]), _bits(eager[i][1][:, :n])), f"replay {i}"
    assert cache.lens.tolist() == eager_cache.lens.tolist() == [103, 98, 21, 44]
