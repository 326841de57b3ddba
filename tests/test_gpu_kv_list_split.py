"""GPU: the listed step call on the paged quantised KV cache with its decode sequences split over the key range
(``sageattention_amd.paged_kv_list_split``, ``sage_kvlsplit_attn``).

``sageattn_kvcache_step_split`` runs every decode sequence (1 .. 32 rows) of a step as S key-range chunks and leaves the longer ones to the listed
call's chunk launch.  Every equality is ``torch.equal`` on the bits; outputs, pool and workspaces are poisoned first.
  A  the rows of a decode sequence of n rows are those of ``sageattn_kvcache_split(q_dense, cache, S, is_causal=True, pack_gqa=True,
     causal_align="bottom_right")`` with a dense q of n rows (one dense call per distinct n, compared on the sequences of that count), the rows of a
     chunk sequence are ``sageattn_kvcache_step_listed``'s, every row no sequence owns keeps its poison -- over 3.20-A's pool (six slots of
     1061 / 700 / 320 / 321 / 1 / 0 keys behind an interleaved table whose unneeded entries hold -1 / num_pages / 2^31 - 1; pages of 64 keys, 17 per
     sequence, and of 128, 9 per sequence: 18 tiles, S 4 gives T = 5 and chunks start mid-page), S 2 / 4 / 17, four sets of query counts, one
     explicit ``q_start`` with rows in front of key 0; ``grid_out`` against the formula;
  B  against the UNSPLIT listed call at the imported bars of tests/test_gpu_split_exact.py; ``num_splits`` None / 1 give the listed call's bits;
  C  capacity 2560 in pages of 64 and 256 keys, S 2 (T = 20) and S 3 (T = 14), rows 1 and 32: lengths chosen with ``loop_plan.split_chunk`` so that
     chunk 0 and a later chunk each run 0, 1 and 2 trips of the six-body loop with every remainder, with chunks past ``len_b`` and behind the
     diagonal (the test asserts what its selection covers);
  D  under ``tests/fence.py``, both fills, the list workspace and the split workspace inside the fence: well-formed and the four malformed prefix
     arrays; a table id of -1 / num_pages at a tile the call reads gives the bits of 0 / num_pages - 1; guards and pool bytes unchanged;
  E  ``append_varlen`` + the call captured once with ``max_seqlen_q`` 130: across three replays a sequence moves from 1 row to 40 rows and a length
     crosses a chunk boundary, each replay equals the eager sequence;
  F  one decode step with S 8 on two streams next to a GEMM, repeated: each repeat equals the first.
"""
import ctypes
import functools
import gc
import random

import pytest
import torch

import loop_plan as lp
from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi, _cabi_kvlist, _cabi_kvlsplit, ops, quant as sq
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    from sageattention_amd.paged_kv_list import sageattn_kvcache_step_listed
    from sageattention_amd.paged_kv_list_split import sageattn_kvcache_step_split
    from sageattention_amd.paged_kv_split import sageattn_kvcache_split
    from sageattention_amd.paged_kv_varlen import append_varlen
    DEV = torch.device("cuda:0")

from test_gpu_paged_kv import _table

F16, BF16 = torch.float16, torch.bfloat16
LENS = (1061, 700, 320, 321, 1, 0)                   # 3.20-A's pool
NB, HKV = len(LENS), 2
ROWS = 1152
PAGINGS = [(64, 17), (128, 9)]                       # (page_size, max_pages_per_seq)
PAGING_IDS = ["page64", "page128"]
NUM_PAGES = 48
PERM = tuple(random.Random(5).sample(range(NUM_PAGES), NUM_PAGES))
POISON = 0x5A
SPLITS = (2, 4, 17)
CASES = [(8, 64, F16), (8, 64, BF16), (8, 128, F16), (8, 128, BF16), (12, 128, BF16), (12, 64, F16), (4, 128, BF16), (4, 64, F16)]
CASE_IDS = [f"hq{h}-d{D}-{'f16' if dt == F16 else 'bf16'}" for h, D, dt in CASES]
# (query counts, max_seqlen_q)
QUERIES = [((1, 5, 32, 1, 1, 1), 32), ((1, 1, 1, 1, 1, 1), 1), ((1, 40, 2, 130, 5, 0), 130), ((40, 1, 3, 0, 32, 33), 33)]
PREFIXES = {"well_formed": [0, 1, 41, 43, 171, 171, 171], "not_monotone": [0, 50, 20, 171, 60, 171, 171], "past_the_end": [0, 1, 2, 3, 900, 2 ** 31 - 1, 171],
            "negative": [-5, -1, 40, -2 ** 31, 100, 171, 171], "all_in_one": [171, 0, 171, 0, 171, 0, 171]}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    """Skips without a GPU; the caches of this file are its own and are dropped on leaving, with the allocator's free blocks (later files reason
    about which block the caching allocator hands out)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi_kvlsplit.load()
    yield
    for f in (_content, _caches, _c_cache):
        f.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _ints(values):
    return torch.tensor(list(values), dtype=torch.int64).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).to(DEV)


def _u8(t):
    return t.contiguous().view(torch.uint8)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _cu(counts):
    out = [0]
    for n in counts:
        out.append(out[-1] + n)
    return out


@functools.lru_cache(maxsize=None)
def _content(D, dt):
    g = torch.Generator().manual_seed(31 + D)
    k = (torch.randn(NB, HKV, ROWS, D, generator=g) + 1.5 * torch.randn(1, HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = (torch.randn(NB, HKV, ROWS, D, generator=g) * (0.25 + torch.rand(1, HKV, 1, D, generator=g))).to(dt).to(DEV)
    return k, v


@functools.lru_cache(maxsize=None)
def _caches(D, dt, paging):
    """The poisoned paged cache of LENS behind the interleaved table: built once, shared, never modified."""
    page_size, max_pages = PAGINGS[paging]
    k, v = _content(D, dt)
    lens = _ints(LENS)
    c = PagedQuantizedKVCache.allocate(NUM_PAGES, page_size, NB, max_pages, HKV, D, dt, DEV)
    for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.k_tail, c.v_tail):
        t.view(torch.uint8).fill_(POISON)
    table = _table(LENS, page_size, max_pages, PERM, NUM_PAGES)
    rest = {p for b, n in enumerate(LENS) for p in table[b][(n + page_size - 1) // page_size:]}
    assert rest == {-1, NUM_PAGES, 2 ** 31 - 1}
    c.block_table.copy_(torch.tensor(table, dtype=torch.int64).to(torch.int32).to(DEV))
    valid = (torch.arange(ROWS, device=DEV)[None, :] < lens[:, None]).view(NB, 1, ROWS, 1)
    c.seed(sq.channel_mean_kvlens(k, lens, "HND"), torch.where(valid, v.abs().float(), 0.0).amax(dim=2))
    c.append(k[:, :, :max(LENS)], v[:, :, :max(LENS)], lens)
    torch.cuda.synchronize()
    assert c.lens.tolist() == list(LENS)
    return c


def _packed_q(Hq, D, dt, counts, slack=0, seed=13):
    g = torch.Generator().manual_seed(seed + D + Hq + sum(counts))
    return torch.randn(sum(counts) + slack, Hq, D, generator=g).to(dt).to(DEV)


def _classes(counts, max_q):
    """(decode sequences, chunk sequences) as (b, first row, rows) by ragged_band's rule on a well-formed prefix array."""
    cu, dec, chk = _cu(counts), [], []
    for b, n in enumerate(counts):
        nb = min(n, max_q)
        if 1 <= nb <= 32:
            dec.append((b, cu[b], nb))
        elif nb > 32:
            chk.append((b, cu[b], nb))
    return dec, chk


def _fenced(fn, *a, **kw):
    """(o, lse) of a call whose outputs and workspaces are the package's ``torch.empty`` bodies, pre-filled with the poison between guards."""
    with Fence(POISON) as f:
        o, lse = fn(*a, return_lse=True, **kw)
        f.check()
        return o.clone(), lse.clone()


def _assert_split(q, cache, counts, max_q, S, what, slack=3, starts=None):
    """The whole property A of one call."""
    nseq, total, cu, Hq, D = len(counts), sum(counts), _cu(counts), q.shape[1], q.shape[2]
    kw = dict(q_start=_ints(starts)) if starts is not None else {}
    o, lse = _fenced(sageattn_kvcache_step_split, q, cache, _ints(cu), max_q, S, **kw)
    assert o.shape == q.shape and lse.shape == (Hq, total + slack) and lse.dtype == torch.float32
    dec, chk = _classes(counts, max_q)
    owned = torch.zeros(total + slack, dtype=torch.bool)
    # decode rows: one dense split call per distinct row count
    for L in sorted({n for _, _, n in dec}):
        qd = torch.zeros(nseq, L, Hq, D, dtype=q.dtype, device=DEV)
        for b, first, n in dec:
            if n == L:
                qd[b] = q[first:first + n]
        dkw = dict(q_start=_ints(starts)) if starts is not None else dict(causal_align="bottom_right")
        od, ld = sageattn_kvcache_split(qd, cache, S, tensor_layout="NHD", is_causal=True, pack_gqa=True, return_lse=True, **dkw)
        for b, first, n in dec:
            if n != L:
                continue
            owned[first:first + n] = True
            do, dl = _bits(o[first:first + n]) != _bits(od[b]), _bits(lse[:, first:first + n]) != _bits(ld[b])
            print(f"{what} decode sequence {b} ({n} rows): o differs in {int(do.sum())} of {do.numel()}, lse in {int(dl.sum())} of {dl.numel()}")
            assert not bool(do.any()), f"{what}: o of decode sequence {b} ({n} rows) differs from the dense split call's in {int(do.sum())} elements"
            assert not bool(dl.any()), f"{what}: lse of decode sequence {b} ({n} rows) differs from the dense split call's in {int(dl.sum())} elements"
            if LENS[b] == 0 and cache.lens[b].item() == 0:
                assert bool((o[first:first + n] == 0).all()) and bool(torch.isneginf(lse[:, first:first + n]).all()), f"{what}: a sequence without keys"
    # chunk rows: the listed call
    ol, ll = _fenced(sageattn_kvcache_step_listed, q, cache, _ints(cu), max_q, **kw)
    for b, first, n in chk:
        owned[first:first + n] = True
        assert torch.equal(_bits(o[first:first + n]), _bits(ol[first:first + n])), f"{what}: o of chunk sequence {b} differs from the listed call's"
        assert torch.equal(_bits(lse[:, first:first + n]), _bits(ll[:, first:first + n])), f"{what}: lse of chunk sequence {b} differs from the listed call's"
    owned = owned.to(DEV)
    assert bool((_u8(o[~owned]) == POISON).all()), f"{what}: rows of o no sequence owns were written"
    # (the returned lse is the kernel's buffer rescaled and corrected on the device: an unwritten word is what the listed call returns for it)
    assert torch.equal(_bits(lse[:, ~owned]), _bits(ll[:, ~owned])), f"{what}: lse of rows no sequence owns was written"
    assert bool(owned.any()) and bool(torch.isfinite(o[owned].float()).all())
    return o, lse


# ---- A: equality on a small pool -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_decode_rows_are_the_dense_splits_and_chunk_rows_the_listed_calls(case, paging):
    Hq, D, dt = case
    cache = _caches(D, dt, paging)
    assert cache.capacity // 64 == (17, 18)[paging] and lp.split_tiles(cache.capacity, 4) == 5
    for counts, max_q in QUERIES:
        q = _packed_q(Hq, D, dt, counts, 3)
        for S in SPLITS:
            _assert_split(q, cache, counts, max_q, S, f"hq {Hq} d{D} {PAGING_IDS[paging]} q {counts}/{max_q} S {S}")
    counts, max_q = QUERIES[0]
    q = _packed_q(Hq, D, dt, counts, 3)
    o = sageattn_kvcache_step_split(q, cache, _ints(_cu(counts)), max_q, 4)                 # without lse: the same o
    assert torch.equal(_bits(o[:sum(counts)]), _bits(sageattn_kvcache_step_split(q, cache, _ints(_cu(counts)), max_q, 4, return_lse=True)[0][:sum(counts)]))


@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
def test_an_explicit_q_start_with_rows_in_front_of_key_0(paging):
    Hq, D, dt = 8, 128, F16
    cache = _caches(D, dt, paging)
    counts = (5, 40, 5, 5, 1, 5)
    starts = [LENS[0] - 5 - 37, 3, -2, 100, -1, 0]        # unaligned; sequences 2 and 4: rows in front of key 0
    q = _packed_q(Hq, D, dt, counts, 3)
    for S in SPLITS:
        _assert_split(q, cache, counts, 130, S, f"q_start {PAGING_IDS[paging]} S {S}", starts=starts)


@pytest.mark.parametrize("Hq", [8, 12, 4])
def test_grid_out_is_pass_2s_grid_plus_the_chunk_grid(Hq):
    D, dt = 64, F16
    cache = _caches(D, dt, 0)
    lib = _cabi_kvlist.load()
    ngb = (Hq // HKV + 3) // 4
    for counts, max_q in QUERIES + [((1, 1, 1, 1, 1, 1), 33)]:
        q = _packed_q(Hq, D, dt, counts)
        total = sum(counts)
        for S in SPLITS:
            probe = ctypes.c_int32(-1)
            with ops.launch_hooks(grid_probe=probe):
                sageattn_kvcache_step_split(q, cache, _ints(_cu(counts)), max_q, S)
            bound = min(NB * ((max_q + 127) // 128), total // 128 + min(NB, total // 33)) if (max_q > 32 and total > 32) else 0
            chunk = 8 * ((Hq % 8) * ((bound + 7) // 8) + (Hq // 8) * bound) if max_q > 32 else 0
            want = 8 * ((NB * S * HKV + 7) // 8) * ngb + chunk
            assert probe.value == want, (counts, max_q, S, probe.value, want)
    ws = lib.sage_kvlist_ws_bytes(NB, 10, 33)
    assert ws > 0


# ---- B: against the unsplit listed call -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
@pytest.mark.parametrize("case", CASES[:4], ids=CASE_IDS[:4])
def test_the_split_matches_the_unsplit_listed_call(case, paging):
    from test_gpu_split_exact import _assert_matches_unsplit
    Hq, D, dt = case
    cache = _caches(D, dt, paging)
    for counts, max_q in (((1, 5, 32, 1, 0, 0), 32), ((1, 40, 2, 130, 0, 0), 130)):          # (slots 0 .. 3: every row sees a key -- the bars compare LSEs by subtraction)
        q = _packed_q(Hq, D, dt, counts)
        cu = _ints(_cu(counts))
        total = sum(counts)
        o0, lse0 = sageattn_kvcache_step_listed(q, cache, cu, max_q, return_lse=True)
        for one in (None, 1):
            o1, lse1 = sageattn_kvcache_step_split(q, cache, cu, max_q, one, return_lse=True)
            assert torch.equal(_bits(o1[:total]), _bits(o0[:total])) and torch.equal(_bits(lse1[:, :total]), _bits(lse0[:, :total])), f"num_splits={one}"
        for S in SPLITS:
            o, lse = sageattn_kvcache_step_split(q, cache, cu, max_q, S, return_lse=True)
            _assert_matches_unsplit(o[:total], lse[:, :total], o0[:total], lse0[:, :total], 0 if dt == F16 else 1, f"q {counts}/{max_q} S{S}")


# ---- C: tile counts ---------------------------------------------------------------------------------------------------------------------------
C_CAP, C_HQ, C_HKV, C_SPLITS, C_PAGES, C_ROWS = 2560, 4, 1, (2, 3), (64, 256), (1, 32)


def _c_keys(lq, case):
    """What a decode sequence of ``lq`` rows, ``case`` = (len, offset), reaches per S: the six-body loop's (trips, remainder) in chunk 0 and in a later
    chunk, and the chunks without work by their cause."""
    n, s = case
    keys = set()
    lenb = min(max(n, 0), C_CAP)
    for S in C_SPLITS:
        for c in range(S):
            p = lp.split_chunk(True, lq, C_CAP, n, s, S, c)
            if p.lk == 0:
                if lenb > 0:
                    keys.add((S, "past_len"))
                continue
            if p.n_iters == 0:
                keys.add((S, "behind_diagonal"))
                continue
            if S == 2:
                keys.add((S, "loop", c, p.trips, p.remainder))
            else:
                keys.add((S, "trips", min(c, 1), p.trips))
    return keys


def _c_wanted():
    w = {(2, "loop", c, t, r) for c in range(2) for t, r in lp.TRIPS_REM} | {(3, "trips", c, t) for c in range(2) for t in (0, 1)}
    return w | {(S, k) for S in C_SPLITS for k in ("past_len", "behind_diagonal")}


def _c_candidates(lq):
    for n in (C_CAP, 1900, 1281, 1000):
        yield (n, n - lq)                                  # bottom-right
        for k in range(-1, 41):
            for e in (0, 37):
                yield (n, 64 * k + e)


@functools.lru_cache(maxsize=None)
def c_cases(lq):
    return lp._greedy(_c_candidates(lq), functools.partial(_c_keys, lq), _c_wanted()) + ((0, 5), (C_CAP, -lq))


def test_the_tile_count_selection_covers_what_it_is_for():
    for lq in C_ROWS:
        cases = c_cases(lq)
        reached = set().union(*(_c_keys(lq, c) for c in cases))
        assert reached >= _c_wanted(), sorted(_c_wanted() - reached, key=repr)
        assert len(cases) <= 64, len(cases)
    assert lp.split_tiles(C_CAP, 2) == 20 and lp.split_tiles(C_CAP, 3) == 14 and (14 >> 2, 14 & 3) == (3, 2)


@functools.lru_cache(maxsize=None)
def _c_cache(D, dt, lq, page_size):
    cases = c_cases(lq)
    nb = len(cases)
    g = torch.Generator().manual_seed(37 + D)
    k = (torch.randn(nb, C_HKV, C_CAP, D, generator=g) + torch.randn(1, C_HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = torch.randn(nb, C_HKV, C_CAP, D, generator=g).to(dt).to(DEV)
    lens = _ints([n for n, _ in cases])
    max_pages = C_CAP // page_size
    num_pages = 2 * nb * max_pages
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(page_size)).tolist()
    table = _table([min(max(n, 0), C_CAP) for n, _ in cases], page_size, max_pages, perm, num_pages)
    c = PagedQuantizedKVCache.from_prefill(k, v, torch.tensor(table, dtype=torch.int64, device=DEV), num_pages, page_size, kv_lens=lens)
    torch.cuda.synchronize()
    assert c.capacity == C_CAP
    return c


@pytest.mark.parametrize("page_size", C_PAGES)
@pytest.mark.parametrize("lq", C_ROWS)
@pytest.mark.parametrize("case", [(64, F16), (128, BF16)], ids=["d64-f16", "d128-bf16"])
def test_every_loop_form_of_a_chunk_is_the_dense_splits(case, lq, page_size):
    D, dt = case
    cases = c_cases(lq)
    nb = len(cases)
    cache = _c_cache(D, dt, lq, page_size)
    g = torch.Generator().manual_seed(lq + D)
    qd = torch.randn(nb, lq, C_HQ, D, generator=g).to(dt).to(DEV)
    q = qd.reshape(nb * lq, C_HQ, D)
    cu = _ints([lq * i for i in range(nb + 1)])
    starts = _ints([s for _, s in cases])
    for S in C_SPLITS:
        want = sageattn_kvcache_split(qd, cache, S, tensor_layout="NHD", is_causal=True, pack_gqa=True, q_start=starts, return_lse=True)
        o, lse = sageattn_kvcache_step_split(q, cache, cu, lq, S, q_start=starts, return_lse=True)
        assert torch.equal(_bits(o.view(nb, lq, C_HQ, D)), _bits(want[0])), f"S{S}: o differs in {int((_bits(o.view(nb, lq, C_HQ, D)) != _bits(want[0])).sum())}"
        assert torch.equal(_bits(lse.view(C_HQ, nb, lq).transpose(0, 1)), _bits(want[1])), f"S{S}: lse differs"
        assert bool(torch.isfinite(o.float()).all())


# ---- D: fence ---------------------------------------------------------------------------------------------------------------------------------
# D 128, Hkv 2, pages of at most 128 keys: Hkv * page_size * D <= 32 KiB, so the page an id of -1 or num_pages would name without the clamp lies
# wholly inside the fence's 64 KiB guard -- a wrong clamp fails the comparison or the guard check and does not fault.
E_LENS, E_PAGES, E_HQ, E_D = (257, 64, 130, 0, 200, 1), 16, 8, 128
E_PERM = (11, 3, 14, 7, 0, 9, 5, 12, 2, 15, 6, 1, 13, 8, 4, 10)
E_PAGINGS = [(64, 5), (128, 3)]


def _e_cache(f, page_size, max_pages, dt):
    nb = len(E_LENS)
    g = torch.Generator().manual_seed(3)
    k = (torch.randn(nb, HKV, 257, E_D, generator=g) + 1.0).to(dt).to(DEV)
    v = torch.randn(nb, HKV, 257, E_D, generator=g).to(dt).to(DEV)
    lens = _ints(E_LENS)
    table = _table(E_LENS, page_size, max_pages, E_PERM, E_PAGES)
    c = PagedQuantizedKVCache.allocate(E_PAGES, page_size, nb, max_pages, HKV, E_D, dt, DEV)
    assert all(f.owns(t) for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.lens))
    c.block_table.copy_(torch.tensor(table, dtype=torch.int64).to(torch.int32).to(DEV))
    c.seed(sq.channel_mean_kvlens(k, lens, "HND"), k.new_ones((nb, HKV, E_D), dtype=torch.float32) * 8.0)
    c.append(k, v, lens)
    torch.cuda.synchronize()
    return c, table


@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
@pytest.mark.parametrize("name", list(PREFIXES))
def test_no_prefix_array_reaches_outside_the_operands_or_the_workspaces(name, fill):
    """q, o, lse, cu_seqlens, the pool, the list workspace and the split workspace in guarded, poisoned memory: whatever the prefix array holds,
    the launches leave every guard its fill and the pool its bytes (the numbers of a malformed call are whatever they are)."""
    dt, total = BF16, 171
    assert HKV * 128 * E_D <= 32 * 1024
    q = _packed_q(E_HQ, E_D, dt, (total,))
    lib, nb = _cabi_kvlist.load(), len(E_LENS)
    for page_size, max_pages in E_PAGINGS:
        with Fence(fill) as f:
            c, _ = _e_cache(f, page_size, max_pages, dt)
            pool = [t.clone() for t in (c.k_int8, c.k_scale, c.v_image)]
            cu = f.input(_ints(PREFIXES[name]))
            qf = f.input(q)
            for max_q, S in ((130, 2), (32, 3), (5, 5)):
                before = len(f.package_allocations())
                o, lse = sageattn_kvcache_step_split(qf, c, cu, max_q, S, return_lse=True)
                torch.cuda.synchronize()
                assert f.owns(o)
                allocs = f.package_allocations()[before:]
                assert ("sageattn_kvcache_step_split", (lib.sage_kvlist_ws_bytes(nb, total, max_q) // 4,), torch.int32) in allocs
                assert ("sageattn_kvcache_step_split", (_cabi.kv_split_ws_bytes(nb, E_HQ, min(max_q, 32), E_D, S) // 4,), torch.float32) in allocs
                assert _cabi_kvlsplit.load().sage_kvlsplit_ws_bytes(nb, E_HQ, max_q, E_D, S) == _cabi.kv_split_ws_bytes(nb, E_HQ, min(max_q, 32), E_D, S)
                f.check()
            for nm, now, was in zip(("k_int8", "k_scale", "v_image"), (c.k_int8, c.k_scale, c.v_image), pool):
                assert torch.equal(_u8(now), _u8(was)), f"{nm}: a pool byte changed"


@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
@pytest.mark.parametrize("paging", range(len(E_PAGINGS)), ids=PAGING_IDS)
def test_a_page_id_outside_the_pool_reads_the_nearest_page_and_nothing_is_written(paging, fill):
    page_size, max_pages = E_PAGINGS[paging]
    dt, S = BF16, 2
    T = lp.split_tiles(page_size * max_pages, S)
    counts = (3, 1, 32, 1, 40, 1)
    q = _packed_q(E_HQ, E_D, dt, counts)
    cu = _ints(_cu(counts))
    with Fence(fill) as f:
        c, table = _e_cache(f, page_size, max_pages, dt)
        set_table = lambda rows: c.block_table.copy_(torch.tensor(rows, dtype=torch.int64).to(torch.int32).to(DEV))
        pool = [t.clone() for t in (c.k_int8, c.k_scale, c.v_image)]
        # (sequence 0, the page of tile T: chunk 1's first tile; sequence 2, page 0: chunk 0's first)
        for b, slot in ((0, (T * 64) // page_size), (2, 0)):
            for bad, near in ((-1, 0), (E_PAGES, E_PAGES - 1)):
                outs = []
                for pid in (bad, near):
                    t = [list(r) for r in table]
                    t[b][slot] = pid
                    set_table(t)
                    o, lse = sageattn_kvcache_step_split(q, c, cu, 40, S, return_lse=True)
                    outs.append((o.clone(), lse.clone()))
                assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1])), \
                    f"sequence {b} slot {slot}: id {bad} against {near}"
        f.check()
        for nm, now, was in zip(("k_int8", "k_scale", "v_image"), (c.k_int8, c.k_scale, c.v_image), pool):
            assert torch.equal(_u8(now), _u8(was)), f"{nm}: a pool byte changed"


# ---- E: graph capture -------------------------------------------------------------------------------------------------------------------------
def test_append_and_the_split_call_capture_into_a_graph():
    """``append_varlen`` + ``sageattn_kvcache_step_split`` captured once with ``max_seqlen_q`` 130 and S 2 on a capacity of 320 (T = 3: chunk 1 begins
    at key 192); replays with other prefix contents written into the captured inputs equal the eager sequence: sequence 0 goes from 1 row to 40
    rows and back to none, and the lengths of sequences 0 and 1 cross key 192 -- 190 -> 191 -> 231 / 190 -> 192 -> 193."""
    Hq, D, dt, page_size, nb, cap, S = 8, 128, BF16, 64, 4, 320, 2
    g = torch.Generator().manual_seed(77)
    k = (torch.randn(nb, HKV, 190, D, generator=g) + 1.0).to(dt).to(DEV)
    v = torch.randn(nb, HKV, 190, D, generator=g).to(dt).to(DEV)
    n0, total, max_rows = (190, 190, 3, 0), 48, 130
    perm = random.Random(11).sample(range(32), 32)
    table = torch.tensor(_table([320, 320, 200, 200], page_size, cap // page_size, perm, 32), dtype=torch.int64, device=DEV)
    assert lp.split_tiles(cap, S) == 3

    def fresh():
        return PagedQuantizedKVCache.from_prefill(k, v, table, 32, page_size, kv_lens=_ints(n0), v_headroom=1.5)

    def step(cache, k_in, v_in, cu_in, q_in):
        append_varlen(cache, k_in, v_in, cu_in, max_rows)
        return sageattn_kvcache_step_split(q_in, cache, cu_in, max_rows, S, return_lse=True)

    steps = []
    for i, counts in enumerate([(1, 2, 0, 40), (40, 1, 3, 4), (0, 33, 15, 0)]):
        g = torch.Generator().manual_seed(60 + i)
        steps.append(((torch.randn(total, HKV, D, generator=g) + 1.0).to(dt).to(DEV), (0.5 * torch.randn(total, HKV, D, generator=g)).to(dt).to(DEV),
                      _ints(_cu(counts)), torch.randn(total, Hq, D, generator=g).to(dt).to(DEV), sum(counts)))
    eager_cache = fresh()
    eager, lens = [], []
    for s in steps:
        eager.append(tuple(t.clone() for t in step(eager_cache, *s[:4])))
        lens.append(eager_cache.lens.tolist())
    assert lens == [[191, 192, 3, 40], [231, 193, 6, 44], [231, 226, 21, 44]]

    warm, cache = fresh(), fresh()
    k_in, v_in, cu_in, q_in = (t.clone() for t in steps[0][:4])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(warm, k_in, v_in, cu_in, q_in)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = step(cache, k_in, v_in, cu_in, q_in)
    for i, (ks, vs, cs, qs, n) in enumerate(steps):
        k_in.copy_(ks), v_in.copy_(vs), cu_in.copy_(cs), q_in.copy_(qs)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(o[:n]), _bits(eager[i][0][:n])) and torch.equal(_bits(lse[:, :n]), _bits(eager[i][1][:, :n])), f"replay {i}"
    assert cache.lens.tolist() == eager_cache.lens.tolist()
    assert any(bool((a[0][:1] != b[0][:1]).any()) for a, b in zip(eager, eager[1:]))          # the replays did follow their inputs


# ---- F: soak ----------------------------------------------------------------------------------------------------------------------------------
SOAK_B, SOAK_HQ, SOAK_HKV, SOAK_CAP, SOAK_ITERS, SOAK_S = 8, 32, 8, 1024, 20, 8


@pytest.mark.parametrize("case", [(128, BF16, 256), (64, F16, 64)], ids=["d128-page256", "d64-page64"])
def test_split_decode_steps_on_two_streams_are_bit_identical(case):
    """One decode step -- one row per sequence, S 8 (T = 2) on a filled paged cache -- alternating between two streams next to a competing GEMM:
    ``o`` and ``lse`` equal the first iteration's, which equal the dense split call's."""
    D, dt, page_size = case
    g = torch.Generator().manual_seed(43 + D)
    q = torch.randn(SOAK_B, SOAK_HQ, D, generator=g).to(dt).to(DEV)
    k = (torch.randn(SOAK_B, SOAK_HKV, SOAK_CAP, D, generator=g) + torch.randn(1, SOAK_HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = torch.randn(SOAK_B, SOAK_HKV, SOAK_CAP, D, generator=g).to(dt).to(DEV)
    have = [1024, 2, 201, 334, 512, 779, 64, 65]
    max_pages = SOAK_CAP // page_size
    num_pages = 2 * SOAK_B * max_pages
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(7)).tolist()
    table = torch.tensor(_table(have, page_size, max_pages, perm, num_pages), dtype=torch.int64, device=DEV)
    c = PagedQuantizedKVCache.from_prefill(k, v, table, num_pages, page_size, kv_lens=_ints(have))
    cu = _ints(range(SOAK_B + 1))

    def step():
        return sageattn_kvcache_step_split(q, c, cu, 1, SOAK_S, return_lse=True)

    first = step()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(first[0].float()).any()) and bool(torch.isfinite(first[1]).all())
    want = sageattn_kvcache_split(q.view(SOAK_B, 1, SOAK_HQ, D), c, SOAK_S, tensor_layout="NHD", is_causal=True, causal_align="bottom_right", pack_gqa=True,
                                  return_lse=True)
    assert torch.equal(_bits(first[0]), _bits(want[0].view(SOAK_B, SOAK_HQ, D))) and torch.equal(_bits(first[1]), _bits(want[1].view(SOAK_B, SOAK_HQ).t()))
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV, dtype=torch.bfloat16)
    bad, last = 0, ""
    for i in range(SOAK_ITERS):
        with torch.cuda.stream(side):
            if i % 4 == 0:
                (a @ a).sum()                      # a competing kernel on the other stream
            r2 = step()
        r1 = step()
        torch.cuda.synchronize()
        for r in (r1, r2):
            if not (torch.equal(r[0], first[0]) and torch.equal(r[1], first[1])):
                bad += 1
                last = f"iteration {i}: o {int((r[0] != first[0]).sum())}, lse {int((r[1] != first[1]).sum())} differ"
    assert bad == 0, f"split step d{D}: {bad} of {2 * SOAK_ITERS} steps differ from the first ({last})"
