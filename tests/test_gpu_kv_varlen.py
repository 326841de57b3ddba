"""GPU: packed, variable-length queries and appends on the paged quantised KV cache (``sageattention_amd.paged_kv_varlen``,
``sage_kvpvarlen_attn`` / ``sage_kvpvarlen_append``).

The ragged kernel runs, per work item, what the dense paged kernel runs at that sample's own ``Lq``, and the ragged append writes what the
dense append of the padded rows writes.  So every property is a bit equality against the existing route:
  A  each sample's rows of ``sageattn_kvcache_varlen`` are the rows of ``sageattn_kvcache(..., is_causal=True, causal_align="bottom_right")``
     on a dense ``q`` of that sample's length -- ``o`` and ``lse``, with and without a window; an empty slot owns no row and nothing around
     the owned rows is written; one case whose items run 1, 2 and 10 tiles behind the new prologue;
  B  a poisoned cache filled by ``append_varlen`` equals byte for byte, in every cache tensor, the twin filled by ``append`` of the zero-padded
     rows with ``new_lens``;
  C  in guarded, poisoned memory a well-formed call and calls with non-monotone, negative and past-``total`` prefix arrays leave every guard
     untouched (wrong numbers are allowed there, an access outside a tensor is not; the clamp's own proof is the host program of
     tests/test_kv_varlen_host.py);
  D  append plus attention captured into a graph: replays with other prefix contents equal the eager sequence.

Shapes: B 4, Hq 8, Hkv 2, D 64 / 128, fp16 / bf16, pages of 64 and 128 keys in a poisoned pool of 32 pages behind an interleaved,
non-ascending table with -1 / ``num_pages`` in unneeded entries, logical capacity 640.
"""
import functools

import pytest
import torch

from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi, quant as sq
    from sageattention_amd.kv_cache import sageattn_kvcache
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    from sageattention_amd.paged_kv_varlen import append_varlen, sageattn_kvcache_varlen
    DEV = torch.device("cuda:0")

B, HQ, HKV, CAP = 4, 8, 2, 640
NUM_PAGES = 32
POISON = 0x5A
F16, BF16 = torch.float16, torch.bfloat16
CASES = [(64, F16), (64, BF16), (128, F16), (128, BF16)]
CASE_IDS = [f"d{D}-{'f16' if dt == F16 else 'bf16'}" for D, dt in CASES]
PAGE_SIZES = (64, 128)
# the pool's pages in the order the table hands them out: a fixed permutation of 0 .. 31
PERM = (19, 3, 30, 7, 0, 25, 9, 12, 28, 2, 15, 22, 6, 1, 31, 13, 8, 4, 27, 10, 17, 24, 5, 20, 11, 29, 14, 21, 16, 26, 18, 23)

CONTEXTS = [(257, 64, 130, 0), (320, 1, 200, 449)]                    # key counts after the append
QUERIES = [(1, 40, 0, 130), (130, 1, 129, 128), (64, 0, 0, 1)]        # a decode row, a chunk inside one block, an empty slot, two query blocks,
WINDOWS = [None, (70, 0)]                                             # more rows than keys, offsets that are and are not multiples of 64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _ints(values):
    return torch.tensor(list(values), dtype=torch.int64).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).to(DEV)


def _u8(t):
    return t.contiguous().view(torch.uint8)


def _table(lens, page_size, max_pages, num_pages=NUM_PAGES):
    """Pages dealt round-robin over the sequences that still need one, from PERM: a sequence's pages interleave with the others' and do not
    ascend; entries no block needs hold -1 and ``num_pages`` in turn."""
    need = [(n + page_size - 1) // page_size for n in lens]
    assert sum(need) <= len(PERM) and max(need) <= max_pages
    rows, it, junk = [[None] * max_pages for _ in lens], iter(PERM), 0
    for slot in range(max_pages):
        for b in range(len(lens)):
            if slot < need[b]:
                rows[b][slot] = next(it)
    for b in range(len(lens)):
        for slot in range(max_pages):
            if rows[b][slot] is None:
                rows[b][slot] = (-1, num_pages)[junk % 2]
                junk += 1
    return rows


def test_the_table_is_what_the_docstring_says():
    t = _table(CONTEXTS[0], 64, CAP // 64)
    used = [p for b, n in enumerate(CONTEXTS[0]) for p in t[b][:(n + 63) // 64]]
    assert len(set(used)) == len(used) == 9 and sorted(PERM) == list(range(NUM_PAGES))
    assert sorted(t[0][:5]) != t[0][:5] and min(t[2][:3]) < max(t[0][:5]) and min(t[0][:5]) < max(t[2][:3])
    assert {p for b, n in enumerate(CONTEXTS[0]) for p in t[b][(n + 63) // 64:]} == {-1, NUM_PAGES}


@functools.lru_cache(maxsize=None)
def _content(D, dt, cap=CAP):
    """k, v ``[B, HKV, cap, D]`` (HND), computed once, never modified."""
    g = torch.Generator().manual_seed(23 + D + cap)
    k = (torch.randn(B, HKV, cap, D, generator=g) + 1.5 * torch.randn(1, HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = (torch.randn(B, HKV, cap, D, generator=g) * (0.25 + torch.rand(1, HKV, 1, D, generator=g))).to(dt).to(DEV)
    return k, v


def _poisoned(D, dt, page_size, lens, cap=CAP):
    """A poisoned paged cache whose table serves ``lens`` keys per sequence, seeded with the statistics of that content, empty."""
    k, v = _content(D, dt, cap)
    c = PagedQuantizedKVCache.allocate(NUM_PAGES, page_size, B, cap // page_size, HKV, D, dt, DEV)
    for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail):
        t.view(torch.uint8).fill_(POISON)
    c.block_table.copy_(_ints([x for row in _table(lens, page_size, cap // page_size) for x in row]).view(B, -1))
    n = _ints(lens)
    valid = (torch.arange(cap, device=DEV)[None, :] < n[:, None]).view(B, 1, cap, 1)
    c.seed(sq.channel_mean_kvlens(k, n, "HND"), torch.where(valid, v.abs().float(), 0.0).amax(dim=2))
    return c


@functools.lru_cache(maxsize=None)
def _cache(D, dt, page_size, ctx, cap=CAP):
    """The cache of context ``ctx`` (one dense append of everything): built once, shared, never modified."""
    k, v = _content(D, dt, cap)
    c = _poisoned(D, dt, page_size, ctx, cap)
    c.append(k, v, _ints(ctx))
    torch.cuda.synchronize()
    assert c.lens.tolist() == list(ctx)
    return c


def _packed_q(D, dt, counts, slack=0, seed=5):
    g = torch.Generator().manual_seed(seed + D + sum(counts))
    return torch.randn(sum(counts) + slack, HQ, D, generator=g).to(dt).to(DEV)


def _cu(counts):
    out = [0]
    for n in counts:
        out.append(out[-1] + n)
    return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _check_against_dense(q, cache, counts, o, lse, window, what):
    """For each distinct length L: the dense bottom-right call on q ``[B, L, Hq, D]`` holding the packed rows of the samples of length L
    (zeros elsewhere); o and lse of those samples are the ragged call's rows, bit for bit."""
    cu = _cu(counts)
    kw = dict(window_size=window) if window is not None else {}
    for L in sorted(set(counts) - {0}):
        qd = torch.zeros(B, L, HQ, q.shape[-1], dtype=q.dtype, device=DEV)
        for b, n in enumerate(counts):
            if n == L:
                qd[b] = q[cu[b]:cu[b + 1]]
        od, ld = sageattn_kvcache(qd, cache, tensor_layout="NHD", is_causal=True, causal_align="bottom_right", return_lse=True, **kw)
        for b, n in enumerate(counts):
            if n != L:
                continue
            do, dl = _bits(o[cu[b]:cu[b + 1]]) != _bits(od[b]), _bits(lse[:, cu[b]:cu[b + 1]]) != _bits(ld[b])
            print(f"{what} sample {b} Lq {L}: o differs in {int(do.sum())} of {do.numel()}, lse in {int(dl.sum())} of {dl.numel()}")
            assert not bool(do.any()), f"{what}: o of sample {b} (Lq {L}) differs in {int(do.sum())} of {do.numel()} elements"
            assert not bool(dl.any()), f"{what}: lse of sample {b} (Lq {L}) differs in {int(dl.sum())} of {dl.numel()} elements"


# ---- A: attention -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", range(len(CONTEXTS)), ids=[f"ctx{i}" for i in range(len(CONTEXTS))])
@pytest.mark.parametrize("page_size", PAGE_SIZES, ids=[f"page{p}" for p in PAGE_SIZES])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_each_samples_rows_are_the_dense_calls(case, page_size, ctx):
    D, dt = case
    cache = _cache(D, dt, page_size, CONTEXTS[ctx])
    for counts in QUERIES:
        slack = 3                                   # rows behind cu[B] that no sample owns: never written
        q = _packed_q(D, dt, counts, slack)
        total, cu = sum(counts), _ints(_cu(counts))
        for window in WINDOWS:
            kw = dict(window_size=window) if window is not None else {}
            with Fence(POISON) as f:                # (o and lse are the package's torch.empty: poisoned bodies between guards)
                o, lse = sageattn_kvcache_varlen(q, cache, cu, max(counts), return_lse=True, **kw)
                f.check()
                o, lse = o.clone(), lse.clone()
            assert o.shape == q.shape and lse.shape == (HQ, total + slack) and lse.dtype == torch.float32
            # an empty slot owns no row (cu[b] == cu[b + 1]); the rows behind the last sample keep the poison: nothing around is written
            assert bool((_u8(o[total:]) == POISON).all()), "rows of o no sample owns were written"
            # (the returned lse is the kernel's buffer rescaled on the device, so only its guards -- f.check() above -- speak for it)
            _check_against_dense(q, cache, counts, o, lse, window, f"ctx {CONTEXTS[ctx]} q {counts} window {window}")
            o_only = sageattn_kvcache_varlen(q, cache, cu, max(counts), **kw)
            assert torch.equal(_bits(o_only[:total]), _bits(o[:total]))


def test_items_of_one_two_and_ten_tiles_behind_the_ragged_prologue():
    """Capacity 1024: the pipelined loop (ten tiles), its last-tile bodies and the general iterations (one and two tiles) behind the new
    prologue, with offsets on and off tile boundaries, at both head sizes."""
    ctx = (64, 128, 640, 601)
    for (D, dt), page_size in (((128, BF16), 64), ((64, F16), 128)):
        cache = _cache(D, dt, page_size, ctx, 1024)
        for counts in ((1, 16, 64, 40), (64, 128, 1, 130)):
            q = _packed_q(D, dt, counts)
            for window in WINDOWS:
                kw = dict(window_size=window) if window is not None else {}
                o, lse = sageattn_kvcache_varlen(q, cache, _ints(_cu(counts)), max(counts), return_lse=True, **kw)
                _check_against_dense(q, cache, counts, o, lse, window, f"cap 1024 d{D} q {counts} window {window}")


def test_q_start_places_the_rows_as_on_the_dense_call():
    """An explicit ``q_start`` (the dense keyword) instead of the bottom-right default, and rows beyond ``max_seqlen_q`` are not computed."""
    D, dt = 128, F16
    cache = _cache(D, dt, 64, CONTEXTS[0])
    counts, start = (40, 40, 40, 40), _ints([200, 3, -7, 0])
    q = _packed_q(D, dt, counts)
    o, lse = sageattn_kvcache_varlen(q, cache, _ints(_cu(counts)), 40, q_start=start, return_lse=True)
    od, ld = sageattn_kvcache(q.view(B, 40, HQ, D), cache, tensor_layout="NHD", is_causal=True, q_start=start, return_lse=True)
    assert torch.equal(_bits(o.view(B, 40, HQ, D)), _bits(od)) and torch.equal(_bits(lse.view(HQ, B, 40).transpose(0, 1)), _bits(ld))
    with Fence(POISON) as f:
        o2 = sageattn_kvcache_varlen(q, cache, _ints(_cu(counts)), 16, q_start=start)
        f.check()
        o2 = o2.clone()
    # (a sample then runs what the dense call runs on its first 16 rows: the rows of a Q scale group that are not loaded count as zeros)
    od16 = sageattn_kvcache(q.view(B, 40, HQ, D)[:, :16], cache, tensor_layout="NHD", is_causal=True, q_start=start)
    for b in range(B):
        assert torch.equal(_bits(o2[40 * b:40 * b + 16]), _bits(od16[b])), "the first max_seqlen_q rows stand where q_start puts them"
        assert bool((_u8(o2[40 * b + 16:40 * b + 40]) == POISON).all()), "rows beyond max_seqlen_q were written"


# ---- B: append --------------------------------------------------------------------------------------------------------------------------
SCHEDULE = [(63, 1, 0, 130), (1, 63, 2, 0), (0, 64, 63, 1)]
FINAL = tuple(sum(s[b] for s in SCHEDULE) for b in range(B))          # (64, 128, 65, 131)
CACHE_TENSORS = ("k_int8", "k_scale", "v_image", "v_scale", "v_amax", "k_mean", "k_tail", "v_tail", "lens", "block_table")


def _nan_rows(n, H, D, dt):
    return torch.full((n, H, D), -1, dtype=torch.int16, device=DEV).view(dt)          # 0xFFFF: NaN as fp16 and as bf16


@pytest.mark.parametrize("page_size", PAGE_SIZES, ids=[f"page{p}" for p in PAGE_SIZES])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_packed_appends_give_the_bytes_of_the_padded_appends(case, page_size):
    D, dt = case
    k, v = _content(D, dt)
    ragged, dense = _poisoned(D, dt, page_size, FINAL), _poisoned(D, dt, page_size, FINAL)
    have = [0] * B
    for counts in SCHEDULE:
        T, cu = max(counts), _cu(counts)
        kp, vp = _nan_rows(sum(counts) + 5, HKV, D, dt), _nan_rows(sum(counts) + 5, HKV, D, dt)      # rows behind total: NaN bits, never read
        kd, vd = torch.zeros(B, HKV, T, D, dtype=dt, device=DEV), torch.zeros(B, HKV, T, D, dtype=dt, device=DEV)
        for b, n in enumerate(counts):
            kp[cu[b]:cu[b + 1]] = k[b, :, have[b]:have[b] + n].transpose(0, 1)
            vp[cu[b]:cu[b + 1]] = v[b, :, have[b]:have[b] + n].transpose(0, 1)
            kd[b, :, :n], vd[b, :, :n] = k[b, :, have[b]:have[b] + n], v[b, :, have[b]:have[b] + n]
        append_varlen(ragged, kp, vp, _ints(cu), T)
        dense.append(kd, vd, _ints(counts))
        have = [h + n for h, n in zip(have, counts)]
        for name in CACHE_TENSORS:
            diff = _u8(getattr(ragged, name)) != _u8(getattr(dense, name))
            assert not bool(diff.any()), f"after {counts}: {name} differs in {int(diff.sum())} bytes"
    assert ragged.lens.tolist() == list(FINAL)
    # the poison is untouched elsewhere: pages the table does not name hold it still
    named = {p for row in _table(FINAL, page_size, CAP // page_size) for p in row if 0 <= p < NUM_PAGES}
    rest = [p for p in range(NUM_PAGES) if p not in named]
    assert rest and all(bool((_u8(t[rest]) == POISON).all()) for t in (ragged.k_int8, ragged.k_scale, ragged.v_image))
    # ... and attention on it is attention on the twin
    counts = (1, 40, 0, 130)
    q = _packed_q(D, dt, counts)
    a = sageattn_kvcache_varlen(q, ragged, _ints(_cu(counts)), 130, return_lse=True)
    b_ = sageattn_kvcache_varlen(q, dense, _ints(_cu(counts)), 130, return_lse=True)
    assert torch.equal(_bits(a[0]), _bits(b_[0])) and torch.equal(_bits(a[1]), _bits(b_[1]))


# ---- C: fence ---------------------------------------------------------------------------------------------------------------------------
# total 171 rows; the malformed arrays break one rule each (and the last one several)
PREFIXES = {
    "well_formed": [0, 1, 41, 41, 171],
    "non_monotone": [0, 120, 30, 171, 60],
    "negative": [-5, -1, 40, -2 ** 31, 100],
    "beyond_total": [0, 100, 5000, 2 ** 31 - 1, 172],
    "everything": [2 ** 31 - 1, -2 ** 31, 171, 0, 2 ** 30],
}


@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
@pytest.mark.parametrize("name", list(PREFIXES))
@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_no_prefix_array_reaches_outside_the_packed_tensors(case, name, fill):
    """q, o, lse, cu_seqlens and the packed new rows in guarded, poisoned memory: whatever the prefix array holds, every guard keeps its fill
    (the numbers of a malformed call are whatever they are)."""
    D, dt = case
    total = 171
    k, v = _content(D, dt)
    cache = _poisoned(D, dt, 64, (450, 450, 450, 450))          # room for every append below: eight pages each, the whole pool
    q = _packed_q(D, dt, (total,))
    with Fence(fill) as f:
        cu = f.input(_ints(PREFIXES[name]))
        qf = f.input(q)
        kn, vn = f.input(k[0, :, :total].transpose(0, 1).contiguous()), f.input(v[0, :, :total].transpose(0, 1).contiguous())
        for window in WINDOWS:
            append_varlen(cache, kn, vn, cu, 130)
            o, lse = sageattn_kvcache_varlen(qf, cache, cu, 130, window_size=window, return_lse=True)
            # (o is the kernel's buffer; the returned lse is that buffer rescaled, so the buffer is looked up among the fence's allocations)
            assert f.owns(o) and ("sageattn_kvcache_varlen", (HQ, total), torch.float32) in f.package_allocations()
            f.check()
    if name == "well_formed":
        assert cache.lens.tolist() == [2, 80, 0, 260]


# ---- D: graph ---------------------------------------------------------------------------------------------------------------------------
def test_append_and_attention_capture_into_a_graph():
    """``append_varlen`` + ``sageattn_kvcache_varlen`` captured once; three replays with other prefix contents and rows written into the
    captured inputs (same total, same maxima) equal the eager sequence, outputs and cache."""
    D, dt, page_size = 128, BF16, 64
    k, v = _content(D, dt)
    n0, total, max_new = (62, 62, 3, 0), 8, 5
    table = _ints([x for row in _table((200, 200, 200, 200), page_size, CAP // page_size) for x in row]).view(B, -1)

    def fresh():
        return PagedQuantizedKVCache.from_prefill(k[:, :, :64], v[:, :, :64], table, NUM_PAGES, page_size, kv_lens=_ints(n0), v_headroom=1.5)

    def step(cache, k_in, v_in, cu_in, q_in):
        append_varlen(cache, k_in, v_in, cu_in, max_new)
        return sageattn_kvcache_varlen(q_in, cache, cu_in, max_new, return_lse=True)

    steps = []
    for i, counts in enumerate([(1, 2, 0, 5), (3, 1, 1, 3), (0, 4, 4, 0)]):
        g = torch.Generator().manual_seed(40 + i)
        steps.append(((torch.randn(total, HKV, D, generator=g) + 1.0).to(dt).to(DEV), (0.5 * torch.randn(total, HKV, D, generator=g)).to(dt).to(DEV),
                      _ints(_cu(counts)), torch.randn(total, HQ, D, generator=g).to(dt).to(DEV)))
    eager_cache = fresh()
    eager = [tuple(t.clone() for t in step(eager_cache, *s)) for s in steps]

    warm, cache = fresh(), fresh()
    k_in, v_in, cu_in, q_in = (t.clone() for t in steps[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(warm, k_in, v_in, cu_in, q_in)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o, lse = step(cache, k_in, v_in, cu_in, q_in)
    for i, (ks, vs, cs, qs) in enumerate(steps):
        k_in.copy_(ks), v_in.copy_(vs), cu_in.copy_(cs), q_in.copy_(qs)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(o), _bits(eager[i][0])) and torch.equal(_bits(lse), _bits(eager[i][1])), f"replay {i}"
    assert cache.lens.tolist() == eager_cache.lens.tolist() == [66, 69, 8, 8]
    assert torch.equal(_u8(cache.v_scale), _u8(eager_cache.v_scale)) and torch.equal(cache.block_table, eager_cache.block_table)
    for b, n in enumerate(cache.lens.tolist()):           # (what a pool holds behind its rows is whatever the allocation held)
        for j in range((n + 63) // 64):
            page, rows = int(table[b, j]), min(64, n - 64 * j)
            for name, sl in (("k_int8", (slice(None), slice(0, rows))), ("k_scale", (slice(None), slice(0, 4))), ("v_image", (slice(None), 0))):
                assert torch.equal(_u8(getattr(cache, name)[page][sl]), _u8(getattr(eager_cache, name)[page][sl])), (name, b, j)
        for name in ("k_tail", "v_tail"):
            assert torch.equal(_u8(getattr(cache, name)[b, :, :n % 64]), _u8(getattr(eager_cache, name)[b, :, :n % 64])), (name, b)
