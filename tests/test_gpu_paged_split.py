"""GPU: the exact split-KV call on the paged quantised KV cache (``sageattention_amd.paged_kv_split``, ``sage_kvpsplit_attn``).

Paging changes addresses and no arithmetic, and a chunk is whole tiles of the LOGICAL key axis, so every property is an equality of bits
against a contiguous ``QuantizedKVCache`` of the same statistics, schedule and capacity (``max_pages_per_seq * page_size``, so that the chunk
length T is the same) called with the same chunk count S.  No tolerance anywhere but in C, which imports its bars.
  A  ``o`` and ``lse`` of ``sageattn_kvcache_split(q, paged, S)`` are those of ``sageattn_kvcache(q, contiguous, num_splits=S)``, and the packed call's
     are the unpacked call's, over a poisoned pool behind a non-ascending, interleaved table whose unneeded entries hold -1 / num_pages / 2^31 - 1;
  B  the two C entries called directly with workspaces of the test's own, filled with a pattern: every byte of ``chunk_max``, ``lse_part`` and
     ``o_part`` equal, the padding between the segments included;
  C  the paged split against the unsplit paged call at the bars of tests/test_gpu_split_exact.py (imported);
  D  a longer pool, lengths and offsets chosen with ``loop_plan.split_chunk`` by the loop forms the chunks then run;
  E  under ``tests/fence.py``, both fills: an id outside the pool at a tile the call reads acts as the nearest page, nothing outside is written;
  F  ``append`` + the split in one captured graph whose replays follow a rewritten table and rewritten lengths;
  G  one decode step with S 8 repeated on two streams next to a competing GEMM.

Shapes of A - C: six samples of 1061 / 700 / 320 / 321 / 1 / 0 keys; pages of 64 keys, 17 per sequence (capacity 1088 = 17 tiles) and of 128 keys, 9
per sequence (capacity 1152 = 18 tiles, where S 4 gives T = 5 and chunks 1 and 3 start in the middle of a page); a pool of 48 pages.
"""
import ctypes
import functools
import random

import pytest
import torch

import loop_plan as lp
from fence import FILLS, Fence
from test_gpu_paged_kv import _bits_equal, _table

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi, _cabi_kvpsplit, core as sc, quant as sq
    from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    from sageattention_amd.paged_kv_split import sageattn_kvcache_split
    DEV = torch.device("cuda:0")

F16, BF16 = torch.float16, torch.bfloat16
LENS = (1061, 700, 320, 321, 1, 0)
NB = len(LENS)
ROWS = 1152                                          # rows of content per sample (the larger capacity)
PAGINGS = [(64, 17), (128, 9)]                       # (page_size, max_pages_per_seq)
PAGING_IDS = ["page64", "page128"]
NUM_PAGES = 48
PERM = tuple(random.Random(5).sample(range(NUM_PAGES), NUM_PAGES))
POISON = 0x5A
SPLITS = (2, 4, 17)
HEADS = [(8, 2), (5, 1)]
HEAD_IDS = ["h8-2", "h5-1"]
CASES = [(64, F16, "HND"), (64, BF16, "NHD"), (128, F16, "NHD"), (128, BF16, "HND")]
CASE_IDS = [f"d{D}-{'f16' if dt == F16 else 'bf16'}-{lay}" for D, dt, lay in CASES]
FORMS = [(lq, pk) for lq in (1, 5, 32) for pk in (True, False)] + [(33, False), (128, False)]        # (Lq, packed)
BR = dict(is_causal=True, causal_align="bottom_right")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()
    yield
    for f in (_content, _caches, _d_caches):
        f.cache_clear()


def _lay(t, layout):
    return t if layout == "HND" else t.transpose(1, 2).contiguous()


def _ints(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _u8(t):
    return t.contiguous().view(torch.uint8)


def _starts(lq):
    """Unaligned offsets, rows in front of key 0 among them: per sample of LENS."""
    return [LENS[0] - lq - 37, -2, 100, LENS[3] - lq, -lq, 0]


def _masks(lq):
    return [("nc", dict()), ("br", BR), ("offsets", dict(is_causal=True, q_start=_ints(_starts(lq))))]


def test_the_shapes_are_what_the_docstring_says():
    for page_size, max_pages in PAGINGS:
        t = _table(LENS, page_size, max_pages, PERM, NUM_PAGES)
        used = [p for b, n in enumerate(LENS) for p in t[b][:(n + page_size - 1) // page_size]]
        assert len(set(used)) == len(used) and all(0 <= p < NUM_PAGES for p in used)
        assert sorted(t[0][:4]) != t[0][:4] and min(t[1][:4]) < max(t[0][:4]) and min(t[0][:4]) < max(t[1][:4])      # not ascending, interleaved
        rest = [p for b, n in enumerate(LENS) for p in t[b][(n + page_size - 1) // page_size:]]
        assert set(rest) == {-1, NUM_PAGES, 2 ** 31 - 1}
    # pages of 128 keys, S 4: T = 5, chunks 1 and 3 start at tiles 5 and 15 -- tile 1 of pages 2 and 7
    cap = PAGINGS[1][0] * PAGINGS[1][1]
    assert cap == 1152 and lp.split_tiles(cap, 4) == 5
    assert [(c * 5) % 2 for c in range(4)] == [0, 1, 0, 1]
    assert lp.split_tiles(PAGINGS[0][0] * PAGINGS[0][1], 17) == 1 and lp.split_tiles(cap, 17) == 2
    assert any(s < 0 for s in _starts(5)) and any(s % 64 for s in _starts(5))


@functools.lru_cache(maxsize=None)
def _content(D, dt, layout, hkv):
    g = torch.Generator().manual_seed(17 + D + hkv)
    k = (torch.randn(NB, hkv, ROWS, D, generator=g) + 1.5 * torch.randn(1, hkv, 1, D, generator=g)).to(dt)
    v = (torch.randn(NB, hkv, ROWS, D, generator=g) * (0.25 + torch.rand(1, hkv, 1, D, generator=g))).to(dt)
    lens = _ints(LENS)
    kd, vd = k.to(DEV), v.to(DEV)
    valid = (torch.arange(ROWS, device=DEV)[None, :] < lens[:, None]).view(NB, 1, ROWS, 1)
    v_amax = torch.where(valid, vd.abs().float(), 0.0).amax(dim=2)
    k, v = _lay(kd, layout), _lay(vd, layout)
    km = sq.channel_mean_kvlens(k, lens, layout)
    return k, v, km, v_amax, lens


@functools.lru_cache(maxsize=None)
def _caches(D, dt, layout, hkv, paging):
    """(contiguous cache, poisoned paged cache) of one content, one set of statistics, one append and one capacity: built once, shared, never
    modified."""
    page_size, max_pages = PAGINGS[paging]
    k, v, km, v_amax, lens = _content(D, dt, layout, hkv)
    ref = QuantizedKVCache.allocate(NB, hkv, page_size * max_pages, D, dt, DEV)
    c = PagedQuantizedKVCache.allocate(NUM_PAGES, page_size, NB, max_pages, hkv, D, dt, DEV)
    for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.k_tail, c.v_tail):
        t.view(torch.uint8).fill_(POISON)
    c.block_table.copy_(torch.tensor(_table(LENS, page_size, max_pages, PERM, NUM_PAGES), dtype=torch.int64).to(torch.int32).to(DEV))
    rows = max(LENS)
    k_rows, v_rows = (t[:, :, :rows] if layout == "HND" else t[:, :rows] for t in (k, v))
    for cache in (ref, c):
        cache.seed(km, v_amax)
        cache.append(k_rows, v_rows, lens, layout)
    torch.cuda.synchronize()
    assert ref.capacity == c.capacity and ref.lens.tolist() == c.lens.tolist() == list(LENS)
    return ref, c


def _q(D, dt, layout, hq, lq, nb=NB, seed=0):
    g = torch.Generator().manual_seed(100 * lq + hq + D + seed)
    return _lay(torch.randn(nb, hq, lq, D, generator=g).to(dt).to(DEV), layout)


# ---- A: the base case -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", range(len(HEADS)), ids=HEAD_IDS)
@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_paged_split_is_the_contiguous_split(case, paging, heads):
    D, dt, layout = case
    hq, hkv = HEADS[heads]
    ref, c = _caches(D, dt, layout, hkv, paging)
    for lq in sorted({lq for lq, _ in FORMS}):
        q = _q(D, dt, layout, hq, lq)
        for mname, mask in _masks(lq):
            for S in SPLITS:
                outs = {}
                for pk in [pk for l_, pk in FORMS if l_ == lq]:
                    kw = dict(tensor_layout=layout, return_lse=True, pack_gqa=pk, **mask)
                    want = sageattn_kvcache(q, ref, num_splits=S, **kw)
                    got = sageattn_kvcache_split(q, c, S, **kw)
                    what = f"lq{lq} {mname} S{S} {'packed' if pk else 'unpacked'}"
                    _bits_equal(got, want, what)
                    assert bool(torch.isfinite(got[0].float()).all()), what
                    assert bool((got[0][5] == 0).all()) and bool(torch.isneginf(got[1][5]).all()), what      # the empty sample reads no entry
                    assert bool(torch.isfinite(got[1][0]).all()), what
                    outs[pk] = got
                if len(outs) == 2:
                    _bits_equal(outs[True], outs[False], f"lq{lq} {mname} S{S}: packed against unpacked")
    # num_splits 1 / None: the unsplit paged call; o alone without return_lse
    q = _q(D, dt, layout, hq, 5)
    plain = sageattn_kvcache(q, c, tensor_layout=layout, return_lse=True, **BR)
    for one in (1, None):
        _bits_equal(sageattn_kvcache_split(q, c, one, tensor_layout=layout, return_lse=True, **BR), plain, f"num_splits={one}")
    o_only = sageattn_kvcache_split(q, c, 4, tensor_layout=layout, **BR)
    assert torch.equal(o_only, sageattn_kvcache(q, ref, num_splits=4, tensor_layout=layout, **BR))
    # on a contiguous cache the new name is the old one with the keyword
    _bits_equal(sageattn_kvcache_split(q, ref, 4, tensor_layout=layout, return_lse=True, **BR),
                sageattn_kvcache(q, ref, num_splits=4, tensor_layout=layout, return_lse=True, **BR), "contiguous cache")


# ---- B: the workspace -------------------------------------------------------------------------------------------------------------------
def _c_call(entry, q, cache, lq, hq, hkv, D, dt, causal, starts, S, ws, gqa_pack):
    o = torch.empty_like(q)
    lse = torch.empty((NB, hq, lq), dtype=torch.float32, device=DEV)
    grid = ctypes.c_int32(-1)
    attr = _cabi.launch_attr(ws, grid_out=grid, q_start=starts, kv_split=S, gqa_pack=gqa_pack)
    _, _, _, _, q_sb, q_sh, q_sl = sq._dims(q, "HND")
    _, _, _, _, k_sb, k_sh, k_sl = sq._dims(cache.k_int8, "HND")
    _, _, _, _, o_sb, o_sh, o_sl = sq._dims(o, "HND")
    code = 0 if dt == F16 else 1
    sm_log2 = sc._sm_log2(D ** -0.5)
    tail = (q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, o_sb, o_sh, o_sl, int(causal), sm_log2, code, code, sq._stream(q), _cabi.attr_arg(attr))
    if entry == "paged":
        rc = _cabi_kvpsplit.load().sage_kvpsplit_attn(
            sq._p(q), sq._p(cache.k_int8), sq._p(cache.v_image), sq._p(o), sq._p(lse), sq._p(cache.k_scale), sq._p(cache.v_scale), sq._p(cache.lens),
            sq._p(cache.block_table), cache.block_table.stride(0), cache.num_pages, cache.page_size, cache.max_pages_per_seq,
            NB, hq, hkv, lq, D, *tail)
        _cabi.check(rc, "sage_kvpsplit_attn")
    else:
        rc = _cabi.load().sage_attn_fused_q_pv_f8_kvlens(
            sq._p(q), sq._p(cache.k_int8), sq._p(cache.v_image), sq._p(o), sq._p(lse), sq._p(cache.k_scale), sq._p(cache.v_scale), None, sq._p(cache.lens),
            NB, hq, hkv, lq, cache.capacity, D, *tail)
        _cabi.check(rc, "sage_attn_fused_q_pv_f8_kvlens")
    torch.cuda.synchronize()
    return o, lse, grid.value


@pytest.mark.parametrize("shape", [(128, BF16, 0, 5, True, True, 7, 1), (64, F16, 1, 33, False, False, 17, 0)], ids=["d128-br-packed-s7", "d64-nc-s17"])
def test_the_split_workspace_is_the_contiguous_calls_byte_for_byte(shape):
    D, dt, heads, lq, causal, packed, S, paging = shape
    hq, hkv = HEADS[heads]
    ref, c = _caches(D, dt, "HND", hkv, paging)
    q = _q(D, dt, "HND", hq, lq)
    starts = (ref.lens.clamp(0, ref.capacity) - lq).to(torch.int32) if causal else None
    nbytes = _cabi.kv_split_ws_bytes(NB, hq, lq, D, S)
    rows = NB * hq * S * lq
    assert (4 * rows) % 128 != 0                       # (the segments end in padding)
    T = lp.split_tiles(c.capacity, S)
    assert paging == 0 or (c.page_size == 128 and T % 2 == 1)      # (pages of two tiles: chunk 1 starts in the middle of a page)
    res = {}
    for entry, cache in (("paged", c), ("contiguous", ref)):
        ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV).view(torch.float32)
        res[entry] = _c_call(entry, q, cache, lq, hq, hkv, D, dt, causal, starts, S, ws, packed) + (ws,)
    (o, lse, grid, ws), (o0, lse0, grid0, ws0) = res["paged"], res["contiguous"]
    assert grid == grid0 == (NB * hkv * ((hq // hkv + 3) // 4) if packed else NB * hq) * S
    _bits_equal((o, lse), (o0, lse0), "the C entries")
    r128 = lambda x: (x + 127) // 128 * 128
    seg = {"chunk_max": (0, 4 * rows), "lse_part": (r128(4 * rows), 4 * rows), "o_part": (2 * r128(4 * rows), 4 * rows * D)}
    a, b = _u8(ws), _u8(ws0)
    for name, (lo, n) in seg.items():
        assert torch.equal(a[lo:lo + n], b[lo:lo + n]), f"{name} differs in {int((a[lo:lo + n] != b[lo:lo + n]).sum())} bytes"
    assert torch.equal(a, b), "the padding differs"
    pad = a[4 * rows:r128(4 * rows)]
    assert pad.numel() > 0 and bool((pad == 0xA5).all())
    cm = ws[:rows].view(NB, hkv, S, hq // hkv, lq)
    assert bool(torch.isneginf(cm[5]).all()) and bool(torch.isfinite(cm[0, :, 0]).all())      # every element written: -inf for the empty sample


# ---- C: against the unsplit paged call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_paged_split_matches_the_unsplit_paged_call(case, paging):
    from test_gpu_split_exact import _assert_matches_unsplit
    D, dt, layout = case
    hq, hkv = HEADS[0]
    _, c = _caches(D, dt, layout, hkv, paging)
    for lq, pk in ((1, True), (32, False), (128, False)):
        q = _q(D, dt, layout, hq, lq)
        for mname, mask in (("nc", dict()), ("br", BR)):
            kw = dict(tensor_layout=layout, return_lse=True, pack_gqa=pk, **mask)
            o0, lse0 = sageattn_kvcache(q, c, **kw)
            for S in SPLITS:
                o, lse = sageattn_kvcache_split(q, c, S, **kw)
                # (samples 0 .. 3: every row sees a key -- the imported bars compare LSEs by subtraction)
                _assert_matches_unsplit(o[:4], lse[:4], o0[:4], lse0[:4], 0 if dt == F16 else 1, f"lq{lq} {mname} S{S}")


# ---- D: loop coverage -------------------------------------------------------------------------------------------------------------------
# Capacity 2560 (40 tiles) in pages of 64 and of 256 keys.  S 2: T = 20, chunks on page boundaries, a chunk's pipelined run reaches 18 -- two trips
# of the six-body loop and every remainder.  S 3: T = 14, chunk 1 starts at tile 14 = tile 2 of page 3 (256-key pages), chunk 2 holds tiles 28 .. 41
# and so reaches past the tensor's 40.  One query block of 16 rows, Hq 4 over Hkv 1 (one packed workgroup), unpacked and packed.
D_CAP, D_LQ, D_HQ, D_HKV, D_SPLITS = 2560, 16, 4, 1, (2, 3)
D_PAGES = (64, 256)


def _d_keys(causal, case):
    """What sample ``case`` = (len, offset) reaches, per S: the loop partition of chunk 0 and of a later chunk, the last-tile bodies, general
    tiles, and the chunks without work by their cause."""
    n, s = case
    keys = set()
    lenb = min(max(n, 0), D_CAP)
    for S in D_SPLITS:
        T = lp.split_tiles(D_CAP, S)
        for c in range(S):
            p = lp.split_chunk(causal, D_LQ, D_CAP, n, s if causal else None, S, c)
            if p.lk == 0:
                if lenb > 0:
                    keys.add((S, "past_len"))
                continue
            if p.n_iters == 0:
                keys.add((S, "behind_diagonal"))
                continue
            if 64 * T * (c + 1) > D_CAP and lenb == D_CAP:
                keys.add((S, "past_tensor"))
            if S == 2:
                keys.add((S, "loop", c, p.trips, p.remainder))
            else:
                keys.add((S, "trips", min(c, 1), p.trips))
            keys.add((S, "last", bool(p.diag_ok if causal else p.tail_ok), p.run > 0))
            piped = (p.run + (2 if p.diag_ok else 0) + (p.n_iters - p.n_steady if p.tail_ok else 0)) if p.entered else 0
            if p.n_iters - piped > 0:
                keys.add((S, "general"))
            if causal and p.run > 0:
                keys.add((S, "diagonal_piped" if p.diag_ok else "diagonal_general"))
    return keys


def _d_wanted(causal):
    w = {(2, "loop", c, t, r) for c in range(2) for t, r in lp.TRIPS_REM} | {(3, "trips", c, t) for c in range(2) for t in (0, 1)}
    w |= {(S, k) for S in D_SPLITS for k in ("past_len", "general")} | {(3, "past_tensor"), (2, "last", True, True), (3, "last", True, True)}
    if causal:
        w |= {(S, k) for S in D_SPLITS for k in ("behind_diagonal", "diagonal_piped", "diagonal_general")} | {(2, "last", False, True)}
    else:
        w |= {(2, "last", True, False), (2, "last", False, False)}
    return w


def _d_candidates(causal):
    if not causal:
        for n in lp.SPLIT_LENS:
            yield (n, None)
        for c in range(3):
            for t in range(15):
                for e in (0, 1, 63):
                    if c * 896 + 64 * t + e <= D_CAP:
                        yield (c * 896 + 64 * t + e, None)
        return
    yield from lp._split_causal_candidates()
    for n in (D_CAP, 1900, 1000):
        for k in range(-1, 41):
            for e in (0, 37):
                yield (n, 64 * k + e)


@functools.lru_cache(maxsize=None)
def d_cases(causal):
    picked = lp._greedy(_d_candidates(causal), functools.partial(_d_keys, causal), _d_wanted(causal))
    return picked + (((0, 5), (D_CAP, -D_LQ)) if causal else ((0, None),))      # a sample without keys; every row in front of key 0


def test_the_loop_selection_covers_what_it_is_for():
    for causal in (False, True):
        cases = d_cases(causal)
        reached = set().union(*(_d_keys(causal, c) for c in cases))
        assert reached >= _d_wanted(causal), sorted(_d_wanted(causal) - reached, key=repr)
        assert len(cases) <= 64, len(cases)
    # S 3: chunk 1 starts at tile 14, which is tile 2 of page 3 of 256 keys, and chunk 2 ends behind the tensor's last tile
    assert lp.split_tiles(D_CAP, 3) == 14 and (14 >> 2, 14 & 3) == (3, 2) and 3 * 14 > D_CAP // 64
    assert lp.split_tiles(D_CAP, 2) == 20 and 20 % 4 == 0


@functools.lru_cache(maxsize=None)
def _d_caches(D, dt, causal, page_size):
    cases = d_cases(causal)
    nb = len(cases)
    g = torch.Generator().manual_seed(29 + D)
    k = (torch.randn(nb, D_HKV, D_CAP, D, generator=g) + torch.randn(1, D_HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = torch.randn(nb, D_HKV, D_CAP, D, generator=g).to(dt).to(DEV)
    lens = _ints([n for n, _ in cases])
    max_pages = D_CAP // page_size
    num_pages = 2 * nb * max_pages
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(page_size)).tolist()
    table = _table([min(max(n, 0), D_CAP) for n, _ in cases], page_size, max_pages, perm, num_pages)
    ref = QuantizedKVCache.from_prefill(k, v, D_CAP, kv_lens=lens)
    c = PagedQuantizedKVCache.from_prefill(k, v, torch.tensor(table, dtype=torch.int64, device=DEV), num_pages, page_size, kv_lens=lens)
    torch.cuda.synchronize()
    assert c.lens.tolist() == ref.lens.tolist() and c.capacity == ref.capacity == D_CAP
    return ref, c


@pytest.mark.parametrize("page_size", D_PAGES)
@pytest.mark.parametrize("causal", (False, True), ids=["nc", "causal"])
@pytest.mark.parametrize("case", [(64, F16), (64, BF16), (128, F16), (128, BF16)], ids=["d64-f16", "d64-bf16", "d128-f16", "d128-bf16"])
def test_every_loop_form_of_a_chunk_is_bit_equal_to_the_contiguous_split(case, causal, page_size):
    D, dt = case
    cases = d_cases(causal)
    ref, c = _d_caches(D, dt, causal, page_size)
    q = _q(D, dt, "HND", D_HQ, D_LQ, nb=len(cases))
    kw = dict(is_causal=True, q_start=_ints([s for _, s in cases])) if causal else dict()
    for S in D_SPLITS:
        for pk in (False, True):
            want = sageattn_kvcache(q, ref, num_splits=S, pack_gqa=pk, return_lse=True, **kw)
            got = sageattn_kvcache_split(q, c, S, pack_gqa=pk, return_lse=True, **kw)
            _bits_equal(got, want, f"S{S} {'packed' if pk else 'unpacked'}")
            assert bool(torch.isfinite(got[0].float()).all())


# ---- E: the device rules ----------------------------------------------------------------------------------------------------------------
# D 128, Hkv 2, pages of at most 128 keys: Hkv * page_size * D <= 32 KiB, so the page an id of -1 or num_pages would name without the clamp lies
# wholly inside the fence's 64 KiB guard -- a wrong clamp fails the comparison or the guard check and does not fault.  No other id is ever put
# where a kernel reads it.  Four samples of 257 / 64 / 130 / 0 keys, pages of 64 keys (five per sequence) and of 128 (three), a pool of 16.
E_LENS, E_PAGES, E_HQ, E_HKV, E_D = (257, 64, 130, 0), 16, 8, 2, 128
E_PERM = (11, 3, 14, 7, 0, 9, 5, 12, 2, 15, 6, 1, 13, 8, 4, 10)
E_PAGINGS = [(64, 5), (128, 3)]


@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
@pytest.mark.parametrize("paging", range(len(E_PAGINGS)), ids=PAGING_IDS)
def test_a_page_id_outside_the_pool_reads_the_nearest_page_and_nothing_is_written(paging, fill):
    page_size, max_pages = E_PAGINGS[paging]
    dt, nb = BF16, len(E_LENS)
    assert E_HKV * page_size * E_D <= 32 * 1024
    g = torch.Generator().manual_seed(3)
    k = (torch.randn(nb, E_HKV, 257, E_D, generator=g) + 1.0).to(dt).to(DEV)
    v = torch.randn(nb, E_HKV, 257, E_D, generator=g).to(dt).to(DEV)
    q = torch.randn(nb, E_HQ, 16, E_D, generator=g).to(dt).to(DEV)
    lens = _ints(E_LENS)
    table = _table(E_LENS, page_size, max_pages, E_PERM, E_PAGES)
    S = 2
    T = lp.split_tiles(page_size * max_pages, S)
    with Fence(fill) as f:
        c = PagedQuantizedKVCache.allocate(E_PAGES, page_size, nb, max_pages, E_HKV, E_D, dt, DEV)
        assert all(f.owns(t) for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.lens))
        set_table = lambda rows: c.block_table.copy_(torch.tensor(rows, dtype=torch.int64).to(torch.int32).to(DEV))
        set_table(table)
        c.seed(sq.channel_mean_kvlens(k, lens, "HND"), k.new_ones((nb, E_HKV, E_D), dtype=torch.float32) * 8.0)
        c.append(k, v, lens)
        torch.cuda.synchronize()
        pool = [t.clone() for t in (c.k_int8, c.k_scale, c.v_image)]
        before = len(f.package_allocations())
        for kw in (dict(), dict(BR, pack_gqa=True)):
            # (sample 0, the page of tile 3: chunk 1's first tile with T = 3; sample 2, page 0: chunk 0's first)
            for b, slot in ((0, (T * 64) // page_size), (2, 0)):
                for bad, near in ((-1, 0), (E_PAGES, E_PAGES - 1)):
                    outs = []
                    for pid in (bad, near):
                        t = [list(r) for r in table]
                        t[b][slot] = pid
                        set_table(t)
                        outs.append(sageattn_kvcache_split(q, c, S, return_lse=True, **kw))
                    _bits_equal(outs[0], outs[1], f"sample {b} slot {slot}: id {bad} against {near} ({kw})")
        f.check()
        nws = _cabi.kv_split_ws_bytes(nb, E_HQ, 16, E_D, S) // 4
        assert ("_attn_fused_q", (nws,), torch.float32) in f.package_allocations()[before:]      # the workspace is one of the fenced allocations
        for name, now, was in zip(("k_int8", "k_scale", "v_image"), (c.k_int8, c.k_scale, c.v_image), pool):
            assert torch.equal(_u8(now), _u8(was)), f"{name}: a pool byte changed"


# ---- F: graph capture -------------------------------------------------------------------------------------------------------------------
def test_append_and_the_split_capture_into_a_graph_that_follows_the_table_and_the_lengths():
    """``append`` + ``sageattn_kvcache_split`` captured on one stream; three replays with new rows, new counts and a REWRITTEN table written into
    the captured inputs are bit-equal to the eager sequence."""
    D, dt, nb, hq, hkv = 128, BF16, 4, 8, 2
    page_size, max_pages, S, num_pages = 64, 5, 2, 32   # capacity 320: five tiles, T = 3 -- chunk 1 begins at tile 3
    g = torch.Generator().manual_seed(9)
    k = (torch.randn(nb, hkv, 320, D, generator=g) + 1.0).to(dt).to(DEV)
    v = torch.randn(nb, hkv, 320, D, generator=g).to(dt).to(DEV)
    lens0 = [190, 190, 3, 0]                            # the replays take samples 0 and 1 over the end of tile 2: 191, 193, 194
    perm = random.Random(11).sample(range(num_pages), num_pages)
    base_table = _table([128] * nb, page_size, max_pages, perm, num_pages)      # tiles 0 and 1 of every sequence: pages perm[0:8]

    def table_of(i):
        """The table in front of step ``i`` (-1: the fill).  The OPEN block's page -- an append re-forms that block whole from the raw rows of the
        tail -- moves to a page nobody holds: tile 2 in front of steps 0 and 1, tile 3 (opened by step 1) in front of step 2."""
        t = [list(r) for r in base_table]
        for b in range(nb):
            t[b][2] = perm[8 + 4 * {-1: 0, 0: 1, 1: 2, 2: 2}[i] + b]
            t[b][3] = perm[20 + 4 * (i == 2) + b]
        return t

    def set_table(c, i):
        c.block_table.copy_(torch.tensor(table_of(i), dtype=torch.int32).to(DEV))

    def fresh():
        c = PagedQuantizedKVCache.allocate(num_pages, page_size, nb, max_pages, hkv, D, dt, DEV)
        for t in (c.k_int8, c.k_scale, c.v_image, c.k_tail, c.v_tail):
            t.view(torch.uint8).fill_(POISON)
        set_table(c, -1)
        lens = _ints(lens0)
        c.seed(sq.channel_mean_kvlens(k[:, :, :190], lens, "HND"), v[:, :, :190].abs().float().amax(dim=2) * 1.5)
        c.append(k[:, :, :190], v[:, :, :190], lens)
        return c

    def step(cache, k_in, v_in, n_in, q_in):
        cache.append(k_in, v_in, n_in)
        return sageattn_kvcache_split(q_in, cache, S, pack_gqa=True, return_lse=True, **BR)

    steps = [(k[:, :, 200 + 2 * i:202 + 2 * i].contiguous(), v[:, :, 200 + 2 * i:202 + 2 * i].contiguous(), _ints(n), _q(D, dt, "HND", hq, 1, nb=nb, seed=20 + i))
             for i, n in enumerate([(1, 1, 1, 0), (2, 2, 0, 1), (1, 0, 2, 2)])]

    eager_cache, eager = fresh(), []
    for i, st in enumerate(steps):
        set_table(eager_cache, i)
        eager.append(tuple(t.clone() for t in step(eager_cache, *st)))
    warm, cache = fresh(), fresh()
    k_in, v_in, n_in, q_in = (t.clone() for t in steps[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(warm, k_in, v_in, n_in, q_in)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = step(cache, k_in, v_in, n_in, q_in)
    for i, (ks, vs, ns, qs) in enumerate(steps):
        k_in.copy_(ks), v_in.copy_(vs), n_in.copy_(ns), q_in.copy_(qs)
        set_table(cache, i)
        graph.replay()
        torch.cuda.synchronize()
        _bits_equal((o, lse), eager[i], f"replay {i}")
    assert cache.lens.tolist() == eager_cache.lens.tolist() == [194, 193, 6, 3]
    # the eager sequence itself is the contiguous cache's, step by step (checked at its end: the same content, the same split)
    ref = QuantizedKVCache.allocate(nb, hkv, page_size * max_pages, D, dt, DEV)
    ref.seed(eager_cache.k_mean, eager_cache.v_amax)
    ref.append(k[:, :, :190], v[:, :, :190], _ints(lens0))
    for st in steps:
        ref.append(*st[:3])
    _bits_equal(eager[-1], sageattn_kvcache(steps[-1][3], ref, num_splits=S, pack_gqa=True, return_lse=True, **BR), "the last step against the contiguous cache")
    assert any(bool((a[0] != b[0]).any()) for a, b in zip(eager, eager[1:]))          # the replays did follow their inputs


# ---- G: soak ----------------------------------------------------------------------------------------------------------------------------
SOAK_B, SOAK_HQ, SOAK_HKV, SOAK_CAP, SOAK_ITERS, SOAK_S = 8, 32, 8, 1024, 20, 8


@pytest.mark.parametrize("case", [(128, BF16, 256), (64, F16, 64)], ids=["d128-page256", "d64-page64"])
def test_split_decode_steps_on_two_streams_are_bit_identical(case):
    """One decode step -- a packed bottom-right call of one row with S 8 (T = 2) on a filled paged cache -- alternating between two streams next to
    a competing GEMM: ``o`` and ``lse`` equal the first iteration's, which equal the contiguous split's."""
    D, dt, page_size = case
    g = torch.Generator().manual_seed(41 + D)
    q = torch.randn(SOAK_B, SOAK_HQ, 1, D, generator=g).to(dt).to(DEV)
    k = (torch.randn(SOAK_B, SOAK_HKV, SOAK_CAP, D, generator=g) + torch.randn(1, SOAK_HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = torch.randn(SOAK_B, SOAK_HKV, SOAK_CAP, D, generator=g).to(dt).to(DEV)
    have = [1024, 2, 201, 334, 512, 779, 64, 65]
    max_pages = SOAK_CAP // page_size
    num_pages = 2 * SOAK_B * max_pages
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(7)).tolist()
    table = torch.tensor(_table(have, page_size, max_pages, perm, num_pages), dtype=torch.int64, device=DEV)
    lens = _ints(have)
    c = PagedQuantizedKVCache.from_prefill(k, v, table, num_pages, page_size, kv_lens=lens)
    ref = QuantizedKVCache.from_prefill(k, v, SOAK_CAP, kv_lens=lens)

    def step():
        return sageattn_kvcache_split(q, c, SOAK_S, pack_gqa=True, return_lse=True, **BR)

    first = step()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(first[0].float()).any()) and bool(torch.isfinite(first[1]).all())
    _bits_equal(first, sageattn_kvcache(q, ref, num_splits=SOAK_S, pack_gqa=True, return_lse=True, **BR), "against the contiguous split")
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
    assert bad == 0, f"paged split step d{D}: {bad} of {2 * SOAK_ITERS} steps differ from the first ({last})"
