"""GPU: the step call on the paged quantised KV cache over device-built work lists (``sageattention_amd.paged_kv_list``, ``sage_kvlist_attn``;
DESIGN 3.23).

``sageattn_kvcache_step_listed`` puts a plan launch in front of the step call's two launches and lets them take their items from its lists,
heaviest first.  The reference is ``sageattn_kvcache_step``, the bar is bit equality, no tolerance:
  A  ``o`` and ``lse`` equal the step call's bits on every owned row and every other row keeps the poison -- over the step tests' cases, queries and
     windows, their explicit ``q_start`` and capacity-1024 cases, and one cache of this file: B 11 (a ragged octet of the decode grid), a sequence
     of three query blocks, seven chunk items over four chunk sequences;
  B  the device's header and both lists are ``sage_kvlist_plan_host``'s on the same words, ``grid_out`` is the sum of the two grids that function
     returns, and for the mixed step that sum is below the step call's dense grids;
  C  in guarded, poisoned memory -- the list workspace included, so every entry behind a list's count holds the fill -- a well-formed call and the
     four malformed prefix arrays leave every guard untouched.  (The issue's further check, a workspace of 0x7f bytes behind a stubbed plan launch,
     would need a test-only entry in the C boundary and is left out: the lists' clamps are read in csrc/sage_attn_body.h, and the plan's own
     bounds are tests/step_list_main.cpp's.);
  D  append plus the call captured into a graph with ``max_seqlen_q`` 130: replays that move a sequence from 1 row to 40 and another from 2 to 33,
     and change which slot holds the longest context, equal the eager sequence.
"""
import ctypes
import gc

import numpy as np
import pytest
import torch

from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi, _cabi_kvlist, ops, quant as sq
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    from sageattention_amd.paged_kv_list import sageattn_kvcache_step_listed
    from sageattention_amd.paged_kv_step import sageattn_kvcache_step
    from sageattention_amd.paged_kv_varlen import append_varlen
    DEV = torch.device("cuda:0")

from test_gpu_kv_varlen import B, BF16, CAP, CONTEXTS, F16, HKV, NUM_PAGES, PAGE_SIZES, POISON, PREFIXES, WINDOWS, _bits, _cache, _content, _cu, _ints, _table, _u8
from test_gpu_kv_step import CASE_IDS, CASES, QUERIES, _owned, _packed_q

HDR = 16
# this file's cache: eleven sequences over 64-key pages, logical capacity 320
B11, CAP11 = 11, 320
COUNTS11 = (1, 130, 1, 0, 33, 1, 2, 40, 1, 32, 260)
CTX11 = (200, 130, 64, 0, 100, 1, 65, 40, 128, 32, 300)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    """Skips without a GPU -- and hands the device's memory back as it was found.  This file runs in front of the files whose shared, cached
    fixtures it borrows (``_cache`` / ``_content`` of test_gpu_kv_varlen.py), so it would build them first, between its own short-lived tensors,
    and leave them standing in blocks with holes: later tests that reason about what the caching allocator hands out (test_gpu_soak_split_cache.py)
    would meet another allocator than on the parent.  If the shared caches were empty on entry they are emptied again, and the allocator's free
    blocks are released; the files behind this one then build their fixtures as they always did."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi_kvlist.load()
    borrowed = _cache.cache_info().currsize == 0 and _content.cache_info().currsize == 0
    yield
    if borrowed:
        _cache.cache_clear()
        _content.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def cache11():
    """B 11, Hkv 2, D 128 bf16, 22 of the pool's 32 pages behind the interleaved table, poisoned elsewhere; built once, never modified."""
    D, dt = 128, BF16
    g = torch.Generator().manual_seed(911)
    k = (torch.randn(B11, HKV, CAP11, D, generator=g) + 1.5 * torch.randn(1, HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = (torch.randn(B11, HKV, CAP11, D, generator=g) * (0.25 + torch.rand(1, HKV, 1, D, generator=g))).to(dt).to(DEV)
    c = PagedQuantizedKVCache.allocate(NUM_PAGES, 64, B11, CAP11 // 64, HKV, D, dt, DEV)
    for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail):
        t.view(torch.uint8).fill_(POISON)
    c.block_table.copy_(_ints([x for row in _table(CTX11, 64, CAP11 // 64) for x in row]).view(B11, -1))
    n = _ints(CTX11)
    valid = (torch.arange(CAP11, device=DEV)[None, :] < n[:, None]).view(B11, 1, CAP11, 1)
    c.seed(sq.channel_mean_kvlens(k, n, "HND"), torch.where(valid, v.abs().float(), 0.0).amax(dim=2))
    c.append(k, v, n)
    torch.cuda.synchronize()
    assert c.lens.tolist() == list(CTX11)
    return c


def _both(q, cache, cu, max_q, **kw):
    """The listed call and the step call on the same operands, each into outputs pre-poisoned by the fence: (o, lse) of each."""
    out = []
    for fn in (sageattn_kvcache_step_listed, sageattn_kvcache_step):
        with Fence(POISON) as f:
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
    assert not bool(do[own].any()), f"{what}: o differs from the step call's in {int(do[own].sum())} elements of owned rows"
    assert not bool(dl[:, own].any()), f"{what}: lse differs from the step call's in {int(dl[:, own].sum())} elements of owned rows"
    assert bool((_u8(o[~own]) == POISON).all()), f"{what}: rows of o no sequence owns were written"
    assert not bool(dl[:, ~own].any()), f"{what}: lse of rows no sequence owns was written"
    assert bool(own.any()) and torch.isfinite(o[own].float()).all()


# ---- A: the step call's bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_row_is_the_step_calls(case):
    Hq, D, dt = case
    for page_size in PAGE_SIZES:
        for ctx in CONTEXTS:
            cache = _cache(D, dt, page_size, ctx)
            for counts, max_q in QUERIES:
                q = _packed_q(Hq, D, dt, counts, 3)
                for window in WINDOWS:
                    kw = dict(window_size=window) if window is not None else {}
                    _assert_same(q, cache, counts, max_q, f"hq {Hq} d{D} page {page_size} ctx {ctx} q {counts}/{max_q} window {window}", **kw)
    cache = _cache(D, dt, PAGE_SIZES[0], CONTEXTS[0])
    counts, max_q = QUERIES[0]
    q = _packed_q(Hq, D, dt, counts, 3)
    o = sageattn_kvcache_step_listed(q, cache, _ints(_cu(counts)), max_q)           # without lse: the same o
    assert torch.equal(_bits(o[:sum(counts)]), _bits(sageattn_kvcache_step(q, cache, _ints(_cu(counts)), max_q)[:sum(counts)]))


def test_an_explicit_q_start_places_the_rows_of_both_lists():
    Hq, D, dt = 8, 128, F16
    cache = _cache(D, dt, 64, CONTEXTS[0])
    counts, start = (1, 40, 20, 130), _ints([200, 3, -7, 0])         # (rows in front of key 0, rows past the last key)
    q = _packed_q(Hq, D, dt, counts, 3)
    for window in WINDOWS:
        _assert_same(q, cache, counts, 130, f"q_start window {window}", q_start=start, window_size=window)
    _assert_same(q, cache, counts, 130, "q_start int", q_start=5)


def test_a_decode_sequence_of_ten_tiles():
    ctx = (64, 128, 640, 601)
    for (Hq, D, dt), page_size in (((12, 128, BF16), 64), ((8, 64, F16), 128)):
        cache = _cache(D, dt, page_size, ctx, 1024)
        for counts in ((16, 40, 1, 130), (1, 1, 32, 2), (64, 2, 128, 1)):
            q = _packed_q(Hq, D, dt, counts, 3)
            for window in WINDOWS:
                kw = dict(window_size=window) if window is not None else {}
                _assert_same(q, cache, counts, max(counts), f"cap 1024 hq {Hq} d{D} q {counts} window {window}", **kw)


def test_eleven_sequences_a_ragged_octet_and_three_query_blocks(cache11):
    Hq, D, dt = 8, 128, BF16
    q = _packed_q(Hq, D, dt, COUNTS11, 3)
    for window in WINDOWS:
        kw = dict(window_size=window) if window is not None else {}
        _assert_same(q, cache11, COUNTS11, 260, f"B 11 window {window}", **kw)
    _assert_same(q, cache11, COUNTS11, 130, "B 11, the longest sequence cut to 130 rows")


# ---- B: the plan and the grid --------------------------------------------------------------------------------------------------------------
def _host_plan(counts, lens, cap, max_q, Hq, D, window=0, Bn=None):
    """sage_kvlist_plan_host on the words the Python layer hands the device: (workspace, decode grid, chunk grid)."""
    Bn = Bn or len(counts)
    lib = _cabi_kvlist.load()
    cu = np.array(_cu(counts), dtype=np.int32)
    kv = np.array(lens, dtype=np.int32)
    start = (np.clip(kv.astype(np.int64), 0, cap) - np.array(counts, dtype=np.int64)).astype(np.int32)      # bottom-right
    nbytes = lib.sage_kvlist_ws_bytes(Bn, sum(counts), max_q)
    ws = np.full(nbytes // 4, -1, dtype=np.int32)
    dg, cg = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.sage_kvlist_plan_host(cu.ctypes.data, kv.ctypes.data, start.ctypes.data, Bn, sum(counts), max_q, cap, window, Hq, HKV, D,
                                   ws.ctypes.data, nbytes, ctypes.byref(dg), ctypes.byref(cg))
    assert rc == 0, lib.sage_last_error()
    return ws, dg.value, cg.value


def _assert_plan(q, cache, counts, max_q, window=None):
    Hq, D = q.shape[1], q.shape[2]
    probe = ctypes.c_int32(-1)
    kw = dict(window_size=window) if window is not None else {}
    with ops.launch_hooks(grid_probe=probe):
        _, ws = sageattn_kvcache_step_listed(q, cache, _ints(_cu(counts)), max_q, return_plan=True, **kw)
    torch.cuda.synchronize()
    want, dg, cg = _host_plan(counts, cache.lens.tolist(), cache.capacity, max_q, Hq, D, window[0] + 1 if window is not None else 0)
    got = ws.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape
    nd, nc = int(want[0]), int(want[1])
    Bn = len(counts)
    assert got[:HDR].tolist() == want[:HDR].tolist(), (counts, max_q, got[:HDR], want[:HDR])
    assert got[HDR:HDR + nd].tolist() == want[HDR:HDR + nd].tolist()
    assert got[HDR + Bn:HDR + Bn + 2 * nc].tolist() == want[HDR + Bn:HDR + Bn + 2 * nc].tolist()
    assert probe.value == dg + cg, (counts, max_q, probe.value, dg, cg)
    return want, dg, cg


@pytest.mark.parametrize("Hq", [8, 12, 4])
def test_the_devices_lists_are_the_host_functions_and_grid_out_is_their_grids(Hq):
    D, dt = 64, F16
    cache = _cache(D, dt, 64, CONTEXTS[0])
    ngb = (Hq // HKV + 3) // 4
    for counts, max_q in QUERIES + [((1, 1, 1, 1), 33), ((1, 1, 1, 1), 129)]:
        q = _packed_q(Hq, D, dt, counts)
        for window in WINDOWS:
            want, dg, cg = _assert_plan(q, cache, counts, max_q, window)
            assert dg == 8 * ((B * HKV + 7) // 8) * ngb and (cg == 0) == (max_q <= 32 or sum(counts) < 33)
            assert int(want[0]) == sum(1 for n in counts if 1 <= min(n, max_q) <= 32)
            assert int(want[1]) == sum((min(n, max_q) + 127) // 128 for n in counts if min(n, max_q) > 32)
    # the mixed step: five chunk slots of Hq heads where the step call starts B * ceil(130 / 128) = 8
    counts, max_q = QUERIES[0]
    _, dg, cg = _assert_plan(_packed_q(Hq, D, dt, counts), cache, counts, max_q)
    parent = B * HKV * ngb + B * Hq * ((max_q + 127) // 128)
    # (Hq 4: no whole head per XCD, the four heads' five items are dealt in one octet each -- 32 workgroups, the step call's number)
    assert dg + cg < parent if Hq >= 8 else dg + cg == parent, (dg, cg, parent)


def test_the_plan_of_eleven_sequences(cache11):
    q = _packed_q(8, 128, BF16, COUNTS11)
    want, dg, cg = _assert_plan(q, cache11, COUNTS11, 260)
    # the bound: min(11 * 3, 501 // 128 + min(11, 501 // 33)) = 14 chunk slots of Hq = 8 heads; three octets of (sequence, kv head) units
    assert int(want[0]) == 6 and int(want[1]) == 7 and dg == 8 * 3 and cg == 8 * 14
    # bottom-right: the decode sequences 0, 6, 8, 2, 5, 9 have contexts 200, 65, 128, 64, 1, 32 -- weights 4, 2, 2, 1, 1, 1, ties by index
    assert want[HDR:HDR + 6].tolist() == [0, 6, 8, 2, 5, 9]
    # the chunk items by the tiles they visit, min(2 j + 2 + ceil((keys - rows) / 64), ceil(keys / 64)): sequence 10 (300 keys, 260 rows) 3, 5, 5;
    # sequence 1 (130, 130) 2, 3; sequence 4 (100, 33) 2; sequence 7 (40, 40) 1 -- equal weights by sequence ascending, then block descending
    assert want[HDR + B11:HDR + B11 + 14].reshape(7, 2).tolist() == [[10, 2], [10, 1], [1, 1], [10, 0], [1, 0], [4, 0], [7, 0]]


# ---- C: fence ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
@pytest.mark.parametrize("name", list(PREFIXES))
@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=[CASE_IDS[0], CASE_IDS[4]])
def test_no_prefix_array_reaches_outside_the_packed_tensors_or_the_workspace(case, name, fill):
    """q, o, lse, cu_seqlens and the list workspace in guarded, poisoned memory: whatever the prefix array holds, the three launches leave every
    guard its fill (the numbers of a malformed call are whatever they are)."""
    Hq, D, dt = case
    total = 171
    cache = _cache(D, dt, 64, CONTEXTS[0])
    q = _packed_q(Hq, D, dt, (total,))
    lib = _cabi_kvlist.load()
    with Fence(fill) as f:
        cu = f.input(_ints(PREFIXES[name]))
        qf = f.input(q)
        for max_q in (130, 32):
            for window in WINDOWS:
                o, lse, ws = sageattn_kvcache_step_listed(qf, cache, cu, max_q, window_size=window, return_lse=True, return_plan=True)
                words = lib.sage_kvlist_ws_bytes(B, total, max_q) // 4
                assert f.owns(o) and f.owns(ws) and ws.shape == (words,)
                assert ("sageattn_kvcache_step_listed", (words,), torch.int32) in f.package_allocations()
                f.check()


# ---- D: graph ------------------------------------------------------------------------------------------------------------------------------
def test_append_and_the_listed_call_capture_into_a_graph():
    """``append_varlen`` + ``sageattn_kvcache_step_listed`` captured once with ``max_seqlen_q`` 130; replays with other prefix contents written into
    the captured inputs equal the eager sequence: sequence 0 goes from 1 row to 40 rows and back to none, sequence 1 from 2 rows to 33, and the
    longest context moves from slot 1 to slot 0 -- the lists are built on the device at every replay."""
    Hq, D, dt, page_size = 8, 128, BF16, 64
    k, v = _content(D, dt)
    n0, total, max_rows = (62, 62, 3, 0), 48, 130
    table = _ints([x for row in _table((200, 200, 200, 200), page_size, CAP // page_size) for x in row]).view(B, -1)

    def fresh():
        return PagedQuantizedKVCache.from_prefill(k[:, :, :64], v[:, :, :64], table, NUM_PAGES, page_size, kv_lens=_ints(n0), v_headroom=1.5)

    def step(cache, k_in, v_in, cu_in, q_in, fn=None):
        append_varlen(cache, k_in, v_in, cu_in, max_rows)
        return (fn or sageattn_kvcache_step_listed)(q_in, cache, cu_in, max_rows, return_lse=True)

    steps = []
    for i, counts in enumerate([(1, 2, 0, 40), (40, 1, 3, 4), (0, 33, 15, 0)]):
        g = torch.Generator().manual_seed(60 + i)
        steps.append(((torch.randn(total, HKV, D, generator=g) + 1.0).to(dt).to(DEV), (0.5 * torch.randn(total, HKV, D, generator=g)).to(dt).to(DEV),
                      _ints(_cu(counts)), torch.randn(total, Hq, D, generator=g).to(dt).to(DEV), sum(counts)))
    eager_cache, step_cache = fresh(), fresh()
    eager, lens = [], []
    for s in steps:
        eager.append(tuple(t.clone() for t in step(eager_cache, *s[:4])))
        lens.append(eager_cache.lens.tolist())
    parent = [tuple(t.clone() for t in step(step_cache, *s[:4], fn=sageattn_kvcache_step)) for s in steps]
    assert lens[0].index(max(lens[0])) == 1 and lens[1].index(max(lens[1])) == 0          # (which slot holds the longest context changes)
    for i, s in enumerate(steps):                  # the eager sequence is the step call's on the rows a sequence owns
        assert torch.equal(_bits(eager[i][0][:s[4]]), _bits(parent[i][0][:s[4]])) and torch.equal(_bits(eager[i][1][:, :s[4]]), _bits(parent[i][1][:, :s[4]]))

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
