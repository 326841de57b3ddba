"""GPU: the quantised KV cache over a pool of pages (``sageattention_amd.paged_kv_cache``, ``sage_kvpaged_append`` / ``sage_kvpaged_attn``).

Paging changes addresses and no arithmetic, so every property is an equality against the contiguous cache of tests/test_gpu_kv_cache.py:
  A  a paged cache holds, at the places its block table names, byte for byte what the contiguous cache of the same statistics and schedule
     holds in each 64-key block, and every other byte of the pool keeps its poison;
  B  ``sageattn_kvcache(q, paged)`` returns bit for bit the ``o`` and ``lse`` of ``sageattn_kvcache(q, contiguous)``;
  C  the same over a longer pool, with lengths, offsets and windows chosen by the loop forms the paged kernels of every form then run;
  D  the device rules: a page id outside the pool that attention reads acts as the nearest page of the pool, an append through one writes
     nothing, and neither touches memory outside the pool (guarded, poisoned memory, both fills);
  E  a sequence slot seeded again and refilled through new pages; append plus attention in a graph whose replays follow a rewritten table;
     one decode step repeated on two streams.

Shapes of A / B / D / E: those of tests/test_gpu_kv_cache.py (B 4, Hq 8, Hkv 2, final lengths 257 / 64 / 130 / 0), pages of 64 keys with five per
sequence and of 128 keys with three, in a pool of 16.  The table is a fixed permutation: the sequences' pages interleave and do not ascend,
and the entries no block needs hold -1, ``num_pages`` and 2^31 - 1 in turn.
"""
import functools

import pytest
import torch

import loop_plan as lp
import test_gpu_kv_cache as base
from fence import FILLS, Fence
from test_gpu_kv_cache import B, BF16, CASE_IDS, CASES, F16, FINAL, HKV, HQ, POISON, SCHEDULES, _hnd, _ints, _lay, _q, _u8

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi
    from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    DEV = torch.device("cuda:0")

NUM_PAGES = 16
PAGINGS = [(64, 5), (128, 3)]                      # (page_size, max_pages_per_seq)
PAGING_IDS = ["page64", "page128"]
PERM = (11, 3, 14, 7, 0, 9, 5, 12, 2, 15, 6, 1, 13, 8, 4, 10)      # the pool's pages in the order the table hands them out
JUNK = (-1, NUM_PAGES, 2 ** 31 - 1)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _table(lens, page_size, max_pages, perm=PERM, num_pages=NUM_PAGES):
    """[len(lens)][max_pages]: the pages are dealt round-robin over the sequences that still need one (slot 0 of every sequence, then slot 1,
    ...), so a sequence's pages interleave with the others' and do not ascend; what no block needs holds the JUNK values in turn."""
    need = [(n + page_size - 1) // page_size for n in lens]
    assert sum(need) <= len(perm) and max(need) <= max_pages
    rows, it, junk = [[None] * max_pages for _ in lens], iter(perm), 0
    for slot in range(max_pages):
        for b in range(len(lens)):
            if slot < need[b]:
                rows[b][slot] = next(it)
    for b in range(len(lens)):
        for slot in range(max_pages):
            if rows[b][slot] is None:
                rows[b][slot] = JUNK[junk % 3] if JUNK[junk % 3] != NUM_PAGES else num_pages
                junk += 1
    return rows


def test_the_table_is_what_the_docstring_says():
    for page_size, max_pages in PAGINGS:
        t = _table(FINAL, page_size, max_pages)
        used = [p for b, n in enumerate(FINAL) for p in t[b][:(n + page_size - 1) // page_size]]
        assert len(set(used)) == len(used) and all(0 <= p < NUM_PAGES for p in used)
        assert t[0][0] > t[0][1] and sorted(t[0][:3]) != t[0][:3]                          # does not ascend
        assert min(t[2][:2]) < max(t[0][:3]) and min(t[0][:3]) < max(t[2][:2])              # interleaves
        rest = [p for b, n in enumerate(FINAL) for p in t[b][(n + page_size - 1) // page_size:]]
        assert set(rest) == set(JUNK)


def _poisoned(D, dt, page_size, max_pages, nseq=B, num_pages=NUM_PAGES, fill=POISON):
    c = PagedQuantizedKVCache.allocate(num_pages, page_size, nseq, max_pages, HKV, D, dt, DEV)
    for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail):
        t.view(torch.uint8).fill_(fill)
    return c


def _set_table(c, rows):
    c.block_table.copy_(torch.tensor(rows, dtype=torch.int64).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).to(DEV))


@functools.lru_cache(maxsize=None)
def _paged(D, dt, layout, name, paging):
    """The poisoned paged cache seeded with the final content's statistics and filled by schedule ``name``: built once, shared, never modified."""
    page_size, max_pages = PAGINGS[paging]
    k, v, km, v_amax = base._content(D, dt, layout)[:4]
    c = _poisoned(D, dt, page_size, max_pages)
    _set_table(c, _table(FINAL, page_size, max_pages))
    c.seed(km, v_amax)
    assert tuple(base._fill(c, k, v, layout, SCHEDULES[name])) == FINAL
    torch.cuda.synchronize()
    return c


def _expected_pool(ref, lens, table, page_size, num_pages, fill, skip=()):
    """(k_int8, k_scale, v_image) of a pool that holds ``fill`` everywhere but where the table places the blocks of the contiguous cache
    ``ref`` that hold rows: the INT8 rows below the length, the block's four scale slots, its whole V tile.  ``skip``: (sample, block) pairs
    that stay unwritten."""
    tpp = page_size // 64
    D = ref.D
    k = torch.full((num_pages, HKV, page_size, D), fill, dtype=torch.uint8, device=DEV).view(torch.int8)
    ks = torch.full((num_pages, HKV, tpp * 4 * 4), fill, dtype=torch.uint8, device=DEV).view(torch.float32)
    vi = torch.full((num_pages, HKV, tpp, D, 64), fill, dtype=torch.uint8, device=DEV)
    for b, n in enumerate(lens):
        for j in range((n + 63) // 64):
            if (b, j) in skip:
                continue
            page, tip, rows = table[b][j // tpp], j % tpp, min(64, n - 64 * j)
            k[page, :, 64 * tip:64 * tip + rows] = ref.k_int8[b, :, 64 * j:64 * j + rows]
            ks[page, :, 4 * tip:4 * tip + 4] = ref.k_scale[b, :, 4 * j:4 * j + 4]
            vi[page, :, tip] = ref.v_image[b, :, j]
    return k, ks, vi


def _pool_equal(c, want, what):
    for name, got, exp in zip(("k_int8", "k_scale", "v_image"), (c.k_int8, c.k_scale, c.v_image), want):
        diff = _u8(got) != _u8(exp)
        assert not bool(diff.any()), f"{what}: {name} differs in {int(diff.sum())} bytes, pages {sorted(set(diff.nonzero()[:, 0].tolist()))}"


# ---- A: bytes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
@pytest.mark.parametrize("name", list(SCHEDULES))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_bytes_are_the_contiguous_caches_bytes(case, name, paging):
    D, dt, layout = case
    page_size, max_pages = PAGINGS[paging]
    ref = base._filled(D, dt, layout, name)
    c = _paged(D, dt, layout, name, paging)
    assert c.capacity == page_size * max_pages and c.lens.tolist() == ref.lens.tolist() == list(FINAL)
    _pool_equal(c, _expected_pool(ref, FINAL, _table(FINAL, page_size, max_pages), page_size, NUM_PAGES, POISON), f"{name}")
    assert torch.equal(c.v_scale.view(torch.int32), ref.v_scale.view(torch.int32)), "v_scale"
    assert torch.equal(_u8(c.k_tail), _u8(ref.k_tail)) and torch.equal(_u8(c.v_tail), _u8(ref.v_tail)), "tails"
    assert torch.equal(c.k_mean, ref.k_mean) and torch.equal(c.v_amax, ref.v_amax)
    assert c.block_table.tolist() == _table(FINAL, page_size, max_pages)      # (never written)


# ---- B: attention -----------------------------------------------------------------------------------------------------------------------
BR = dict(is_causal=True, causal_align="bottom_right")
MASKS = [dict(), dict(is_causal=True), BR, dict(BR, window_size=(70, 0))]
VARIANTS = [(lq, dict(m, **p)) for lq in (1, 16, 40) for m in MASKS for p in ([dict()] + ([dict(pack_gqa=True)] if lq <= 32 else []))]
VARIANT_IDS = [f"lq{lq}-" + ("-".join(f"{k_}={v_}" for k_, v_ in kw.items()) or "plain").replace(" ", "") for lq, kw in VARIANTS]


def _bits_equal(got, want, what):
    for name, a, b_ in zip(("o", "lse"), got, want):
        ia, ib = a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32), b_.contiguous().view(torch.int16 if b_.element_size() == 2 else torch.int32)
        assert a.shape == b_.shape and torch.equal(ia, ib), f"{what}: {name} differs in {int((ia != ib).sum())} of {ia.numel()} elements"


@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
@pytest.mark.parametrize("variant", range(len(VARIANTS)), ids=VARIANT_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_attention_is_the_contiguous_caches(case, variant, paging):
    D, dt, layout = case
    lq, kw = VARIANTS[variant]
    q = _q(D, dt, layout, lq)
    want = sageattn_kvcache(q, base._filled(D, dt, layout, "one"), tensor_layout=layout, return_lse=True, **kw)
    for name in ("one", "mixed"):
        got = sageattn_kvcache(q, _paged(D, dt, layout, name, paging), tensor_layout=layout, return_lse=True, **kw)
        _bits_equal(got, want, name)
        assert bool((got[0][3] == 0).all()) and bool((got[1][3] == float("-inf")).all())        # the empty sample reads no entry
    o_only = sageattn_kvcache(q, _paged(D, dt, layout, "one", paging), tensor_layout=layout, **kw)
    assert torch.equal(o_only, want[0])


# ---- C: loop forms ----------------------------------------------------------------------------------------------------------------------
# Capacity 1024 (sixteen tiles), Lq 16 (one query block; pack_gqa's limit is 32), B 8, pages of 64 and of 256 keys.  Four calls per cache, one
# per member of the kv_lens family -- lengths non-causal, causal top-left, query offsets, a window on top -- each unpacked and with packed GQA
# groups, for fp16 and bf16 q at both head sizes: the paged kernels of all 2 x 16 forms.  (length, offset) per sample; loop_plan.dense says
# which loop forms each runs, and the test asserts what the selection covers.
C_CAP, C_LQ, C_B = 1024, 16, 8
C_CALLS = {
    "lens":    (dict(), [(512, None), (581, None), (640, None), (767, None), (768, None), (833, None), (64, None), (100, None)], 0),
    "causal":  (dict(is_causal=True), [(64, None), (100, None), (128, None), (300, None), (0, None), (1, None), (65, None), (1024, None)], 0),
    # offsets: bottom-right (len - Lq, a diagonal that crosses tiles: general iterations) and len - 64 on whole tiles (the diag_ok bodies)
    "offsets": (dict(is_causal=True), [(528, 512), (592, 576), (656, 640), (720, 704), (784, 768), (848, 832), (256, 192), (320, 256)], 0),
    "window":  (dict(is_causal=True, window_size=(599, 0)), [(1000, 984), (1024, 1008), (900, 884), (700, 684), (650, 634), (601, 585), (300, 284), (64, 48)], 600),
}
C_WANT = {
    "lens": {"tail", "ragged", "general", "tiles1", "tiles2"} | {f"rem{r}" for r in range(6)},
    "causal": {"tiles1", "tiles2", "general", "ragged"},
    "offsets": {"diag", "general", "ragged"} | {f"rem{r}" for r in range(6)},
    "window": {"head", "head_off_page", "general", "ragged", "rem0", "tiles1"},
}


def _reached(call, page_tiles=4):
    kw, samples, W = C_CALLS[call]
    out = set()
    for n, s in samples:
        p = lp.dense(128, bool(kw.get("is_causal")), C_LQ, C_CAP, n, s if s is not None else (0 if W else None), W, 0)
        if p.n_iters in (1, 2):
            out.add(f"tiles{p.n_iters}")
        if p.entered and p.trips >= 1:
            out.add(f"rem{p.remainder}")
        out |= ({"diag"} if p.diag_ok else set()) | ({"tail"} if p.tail_ok else set())
        if p.lk % 64 and p.n_iters * 64 > p.lk:
            out.add("ragged")
        piped = (p.run + (2 if p.diag_ok else 0) + (p.n_iters - p.n_steady if p.tail_ok else 0)) if p.entered else 0
        if p.n_iters - p.nh - piped > 0:
            out.add("general")
        if p.nh > 0:
            out |= {"head"} | ({"head_off_page"} if (p.kc0 // 64) % page_tiles else set())
    return out


def test_the_loop_form_selection_covers_what_it_is_for():
    for call in C_CALLS:
        assert _reached(call) >= C_WANT[call], (call, sorted(C_WANT[call] - _reached(call)))


@functools.lru_cache(maxsize=None)
def _c_content(D, dt):
    g = torch.Generator().manual_seed(23 + D)
    k = (torch.randn(C_B, HKV, C_CAP, D, generator=g) + 1.5 * torch.randn(1, HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = (torch.randn(C_B, HKV, C_CAP, D, generator=g) * (0.25 + torch.rand(1, HKV, 1, D, generator=g))).to(dt).to(DEV)
    q = torch.randn(C_B, HQ, C_LQ, D, generator=g).to(dt).to(DEV)
    return q, k, v


@pytest.mark.parametrize("page_size", (64, 256))
@pytest.mark.parametrize("call", list(C_CALLS))
@pytest.mark.parametrize("case", [(64, F16), (64, BF16), (128, F16), (128, BF16)], ids=["d64-f16", "d64-bf16", "d128-f16", "d128-bf16"])
def test_every_loop_form_is_bit_equal_to_the_contiguous_cache(case, call, page_size):
    D, dt = case
    kw, samples, _ = C_CALLS[call]
    q, k, v = _c_content(D, dt)
    lens = _ints([n for n, _ in samples])
    if samples[0][1] is not None:
        kw = dict(kw, q_start=_ints([s for _, s in samples]))
    max_pages = C_CAP // page_size
    num_pages = 2 * C_B * max_pages
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(page_size)).tolist()
    table = _table([n for n, _ in samples], page_size, max_pages, perm, num_pages)
    ref = QuantizedKVCache.from_prefill(k, v, C_CAP, kv_lens=lens)
    c = PagedQuantizedKVCache.from_prefill(k, v, torch.tensor(table, dtype=torch.int64, device=DEV), num_pages, page_size, kv_lens=lens)
    assert c.lens.tolist() == ref.lens.tolist()
    for pack in (dict(), dict(pack_gqa=True)):
        want = sageattn_kvcache(q, ref, return_lse=True, **kw, **pack)
        got = sageattn_kvcache(q, c, return_lse=True, **kw, **pack)
        _bits_equal(got, want, f"{call} {pack}")
        assert bool(torch.isfinite(want[0].float()).all())


# ---- D: the device rules ----------------------------------------------------------------------------------------------------------------
# D 128, Hkv 2, pages of at most 128 keys: Hkv * page_size * D <= 32 KiB, so the page an id of -1 or num_pages would name without the clamp
# lies wholly inside the fence's 64 KiB guard -- a wrong clamp fails the comparison or the guard check and does not fault.  No other id is
# ever put where the kernel reads it.
D_CASE = (128, BF16, "HND")


@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
def test_a_page_id_outside_the_pool_reads_the_nearest_page_and_writes_nothing(paging, fill):
    D, dt, layout = D_CASE
    page_size, max_pages = PAGINGS[paging]
    assert HKV * page_size * D <= 32 * 1024
    k, v, km, v_amax = base._content(D, dt, layout)[:4]
    ref = base._filled(D, dt, layout, "one")
    table = _table(FINAL, page_size, max_pages)
    q = _q(D, dt, layout, 16)
    with Fence(fill) as f:
        c = PagedQuantizedKVCache.allocate(NUM_PAGES, page_size, B, max_pages, HKV, D, dt, DEV)
        assert all(f.owns(t) for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.k_tail, c.v_tail, c.lens))
        _set_table(c, table)
        c.seed(km, v_amax)
        base._fill(c, k, v, layout, SCHEDULES["one"])
        _pool_equal(c, _expected_pool(ref, FINAL, table, page_size, NUM_PAGES, fill), "filled under the fence")
        # attention: the id of a tile that is read, replaced by -1 / num_pages, against 0 / num_pages - 1 in its place
        for kw in (dict(), dict(BR, pack_gqa=True)):
            for b, slot in ((0, 1), (2, 0)):
                for bad, near in ((-1, 0), (NUM_PAGES, NUM_PAGES - 1)):
                    outs = []
                    for pid in (bad, near):
                        t = [list(r) for r in table]
                        t[b][slot] = pid
                        _set_table(c, t)
                        outs.append(sageattn_kvcache(q, c, return_lse=True, **kw))
                    _bits_equal(outs[0], outs[1], f"sample {b} slot {slot}: id {bad} against {near} ({kw})")
        f.check()
        # append: blocks behind such entries are not written, the others are, the lengths advance
        c2 = PagedQuantizedKVCache.allocate(NUM_PAGES, page_size, B, max_pages, HKV, D, dt, DEV)
        t = [list(r) for r in table]
        t[0][1], t[2][0] = -1, NUM_PAGES
        _set_table(c2, t)
        c2.seed(km, v_amax)
        base._fill(c2, k, v, layout, SCHEDULES["mixed"])
        torch.cuda.synchronize()
        f.check()
        tpp = page_size // 64
        skip = {(b, j) for b, slot in ((0, 1), (2, 0)) for j in range(slot * tpp, slot * tpp + tpp)}
        _pool_equal(c2, _expected_pool(ref, FINAL, table, page_size, NUM_PAGES, fill, skip), "append through ids outside the pool")
        assert c2.lens.tolist() == list(FINAL)


# ---- E: slots, graph, soak --------------------------------------------------------------------------------------------------------------
def test_a_slot_seeded_again_is_a_fresh_caches_slot():
    """``seed(slots=[1])`` on a filled cache and a refill of slot 1 through new pages: the other slots' bytes and outputs stay, slot 1 is what a
    fresh cache holds and returns."""
    D, dt, layout = 128, F16, "NHD"
    page_size, max_pages = PAGINGS[0]
    k, v, km, v_amax = base._content(D, dt, layout)[:4]
    table = _table(FINAL, page_size, max_pages)
    c = _poisoned(D, dt, page_size, max_pages)
    _set_table(c, table)
    c.seed(km, v_amax)
    base._fill(c, k, v, layout, SCHEDULES["one"])
    q = _q(D, dt, layout, 16)
    kw = dict(tensor_layout=layout, return_lse=True, pack_gqa=True, **BR)
    before = sageattn_kvcache(q, c, **kw)
    pool_before = [t.clone() for t in (c.k_int8, c.k_scale, c.v_image)]
    # slot 1's new content: 100 rows of sample 2's keys and values from row 150 on, statistics of their own, pages nobody holds
    n_new, new_pages = 100, [8, 4]
    assert not set(new_pages) & {p for b, n in enumerate(FINAL) for p in table[b][:(n + 63) // 64]}
    counts = [0, n_new, 0, 0]
    kh, vh = _hnd(k, layout), _hnd(v, layout)
    k_rows = _lay(kh[2:3, :, 150:150 + n_new].expand(B, -1, -1, -1).contiguous(), layout)
    v_rows = _lay(vh[2:3, :, 150:150 + n_new].expand(B, -1, -1, -1).contiguous(), layout)
    km1 = kh[2:3, :, 150:150 + n_new].float().mean(dim=2).to(dt)
    va1 = vh[2:3, :, 150:150 + n_new].abs().float().amax(dim=2) * 1.5
    new_table = [list(r) for r in table]
    new_table[1][:2] = new_pages
    c.seed(km1, va1, slots=[1])
    assert c.lens.tolist() == [FINAL[0], 0, FINAL[2], FINAL[3]]
    _set_table(c, new_table)
    c.append(k_rows, v_rows, _ints(counts), layout)
    km_all, va_all = km.clone(), v_amax.clone()
    km_all[1], va_all[1] = km1[0], va1[0]
    fresh = _poisoned(D, dt, page_size, max_pages)
    _set_table(fresh, new_table)
    fresh.seed(km_all, va_all)
    fresh.append(k_rows, v_rows, _ints(counts), layout)
    assert c.lens.tolist() == [FINAL[0], n_new, FINAL[2], FINAL[3]] and fresh.lens.tolist() == counts
    after, want1 = sageattn_kvcache(q, c, **kw), sageattn_kvcache(q, fresh, **kw)
    for b in (0, 2, 3):          # (the batch is the first dimension of o in both layouts)
        _bits_equal((after[0][b], after[1][b]), (before[0][b], before[1][b]), f"slot {b} after slot 1 was re-seeded")
    _bits_equal((after[0][1], after[1][1]), (want1[0][1], want1[1][1]), "slot 1 against a fresh cache")
    for name, now, was, new in zip(("k_int8", "k_scale", "v_image"), (c.k_int8, c.k_scale, c.v_image), pool_before, (fresh.k_int8, fresh.k_scale, fresh.v_image)):
        others = [p for p in range(NUM_PAGES) if p not in new_pages]
        assert torch.equal(_u8(now[others]), _u8(was[others])), f"{name}: a page outside slot 1's new ones changed"
        assert torch.equal(_u8(now[new_pages]), _u8(new[new_pages])), f"{name}: slot 1's new pages differ from a fresh cache's"
    assert torch.equal(c.v_scale[1].view(torch.int32), fresh.v_scale[1].view(torch.int32))
    assert torch.equal(_u8(c.k_tail[1, :, :n_new % 64]), _u8(fresh.k_tail[1, :, :n_new % 64]))


def test_append_and_attention_capture_into_a_graph_that_follows_the_table():
    """``append`` + ``sageattn_kvcache`` captured on one stream; three replays with new rows, new counts and a REWRITTEN table written into the
    captured inputs are bit-equal to the eager sequence, outputs and pool."""
    D, dt, layout = 128, BF16, "HND"
    page_size, max_pages = PAGINGS[0]
    k, v = base._content(D, dt, layout)[:2]
    n0 = 62          # the replays take the open block over a block end: 62 -> 63 -> 65 -> 66
    lens0 = [n0, n0, 3, 0]
    table0 = _table([128] * B, page_size, max_pages)             # two pages each; every step below rewrites where block 1 goes

    def fresh():
        c = _poisoned(D, dt, page_size, max_pages)
        _set_table(c, table0)
        lens = _ints(lens0)
        c.seed(base.sq.channel_mean_kvlens(k[:, :, :n0], lens, layout), v[:, :, :n0].abs().float().amax(dim=2) * 1.5)
        c.append(k[:, :, :n0], v[:, :, :n0], lens)
        return c

    def step(cache, k_in, v_in, n_in, q_in):
        cache.append(k_in, v_in, n_in)
        return sageattn_kvcache(q_in, cache, pack_gqa=True, return_lse=True, **BR)

    def table_of(i):      # block 1 of every sequence moves to another free page before step i
        t = [list(r) for r in table0]
        for b in range(B):
            t[b][1] = PERM[8 + (b + i) % 4]
        return t

    steps = [(k[:, :, 100 + 2 * i:102 + 2 * i], v[:, :, 100 + 2 * i:102 + 2 * i], _ints(n), _q(D, dt, layout, 1, seed=20 + i))
             for i, n in enumerate([(1, 1, 1, 0), (2, 2, 0, 1), (1, 0, 2, 2)])]
    assert {p for r in table0 for p in r[:2]}.isdisjoint(PERM[8:12])
    eager_cache, eager = fresh(), []
    for i, s in enumerate(steps):
        _set_table(eager_cache, table_of(i))
        eager.append(tuple(t.clone() for t in step(eager_cache, *s)))
    warm, cache = fresh(), fresh()
    k_in, v_in, n_in, q_in = (t.clone() for t in steps[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(warm, k_in, v_in, n_in, q_in)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o, lse = step(cache, k_in, v_in, n_in, q_in)
    for i, (ks, vs, ns, qs) in enumerate(steps):
        k_in.copy_(ks), v_in.copy_(vs), n_in.copy_(ns), q_in.copy_(qs)
        _set_table(cache, table_of(i))
        g.replay()
        torch.cuda.synchronize()
        _bits_equal((o, lse), eager[i], f"replay {i}")
    assert cache.lens.tolist() == eager_cache.lens.tolist() == [n0 + 4, n0 + 3, 6, 3]
    for name in ("k_int8", "k_scale", "v_image", "v_scale", "k_tail", "v_tail"):       # (both pools were poisoned: equal everywhere)
        assert torch.equal(_u8(getattr(cache, name)), _u8(getattr(eager_cache, name))), name


SOAK_B, SOAK_HQ, SOAK_HKV, SOAK_CAP, SOAK_ITERS = 8, 32, 8, 1024, 20


@pytest.mark.parametrize("case", [(128, BF16, 256), (64, F16, 64)], ids=["d128-page256", "d64-page64"])
def test_decode_steps_on_two_streams_are_bit_identical(case):
    """tests/test_gpu_soak_split_cache.py's KV-cache step on a paged cache: prefill, one appended row, one packed bottom-right decode call,
    alternating between two streams next to a competing GEMM; ``o``, ``lse`` and the pool's defined bytes equal the first iteration's.  (A missing
    wait state on the table lookup's way into the tile loads would show here as a difference on some launch.)"""
    D, dt, page_size = case
    g = torch.Generator().manual_seed(41 + D)
    q = torch.randn(SOAK_B, SOAK_HQ, 1, D, generator=g).to(dt).to(DEV)
    k = (torch.randn(SOAK_B, SOAK_HKV, SOAK_CAP, D, generator=g) + torch.randn(1, SOAK_HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = torch.randn(SOAK_B, SOAK_HKV, SOAK_CAP, D, generator=g).to(dt).to(DEV)
    have = [1023, 1, 200, 333, 511, 778, 63, 64]          # a lone key, an open block one row short of its end, a block end, ragged ones between
    after = [n + 1 for n in have]
    max_pages = SOAK_CAP // page_size
    num_pages = 2 * SOAK_B * max_pages
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(7)).tolist()
    rows_t = _table(after, page_size, max_pages, perm, num_pages)
    table = torch.tensor(rows_t, dtype=torch.int64, device=DEV)
    lens0 = _ints(have)
    new = torch.stack([k[b, :, n:n + 1] for b, n in enumerate(have)]), torch.stack([v[b, :, n:n + 1] for b, n in enumerate(have)])
    tpp = page_size // 64

    def defined(c):
        parts = [c.v_scale, c.lens]
        for b, n in enumerate(after):
            for j in range((n + 63) // 64):
                page, tip, r = rows_t[b][j // tpp], j % tpp, min(64, n - 64 * j)
                parts += [c.k_int8[page, :, 64 * tip:64 * tip + r], c.k_scale[page, :, 4 * tip:4 * tip + 4], c.v_image[page, :, tip]]
            parts += [c.k_tail[b, :, :n % 64], c.v_tail[b, :, :n % 64]]
        return torch.cat([t.reshape(-1).view(torch.uint8) for t in parts])

    def step():
        c = PagedQuantizedKVCache.from_prefill(k, v, table, num_pages, page_size, kv_lens=lens0)
        c.append(*new)
        o, lse = sageattn_kvcache(q, c, pack_gqa=True, return_lse=True, **BR)
        return o, lse, defined(c), c

    first = step()
    torch.cuda.synchronize()
    assert first[3].lens.tolist() == after
    assert not bool(torch.isnan(first[0].float()).any()) and bool(torch.isfinite(first[1]).all())
    ref = QuantizedKVCache.from_prefill(k, v, SOAK_CAP, kv_lens=lens0)
    ref.append(*new)
    _bits_equal(first[:2], sageattn_kvcache(q, ref, pack_gqa=True, return_lse=True, **BR), "against the contiguous cache")
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
            if not (torch.equal(r[0], first[0]) and torch.equal(r[1], first[1]) and torch.equal(r[2], first[2])):
                bad += 1
                last = f"iteration {i}: o {int((r[0] != first[0]).sum())}, lse {int((r[1] != first[1]).sum())}, pool bytes {int((r[2] != first[2]).sum())} differ"
    assert bad == 0, f"paged step d{D}: {bad} of {2 * SOAK_ITERS} steps differ from the first ({last})"
