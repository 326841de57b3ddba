"""GPU: forked sequences of the paged quantised KV cache (``PagedQuantizedKVCache.fork``, ``sage_kvfork``).

A fork copies and computes nothing new, so every property is an equality:
  A  after one ``fork`` of all parents every pool byte, table entry, per-slot tensor and length is what tests/ref_kvfork.py says (asserted
     against hand-written cases in tests/test_kvfork_host.py); everything else keeps its poison, the parents keep their bits;
  B  ``sageattn_kvcache`` on a child returns bit for bit the ``o`` and ``lse`` of its parent, and the parents' outputs do not change;
  C  parent and child then append different rows: each equals, block by block through its table and in ``o`` / ``lse``, a contiguous
     ``QuantizedKVCache`` seeded with the parent's statistics and filled with that sequence's own rows; shared pages keep their bytes;
  D  ``prefix_lens``: the child equals a contiguous cache of the parent's first ``P`` rows (``P`` rounded down to a block when below ``L``);
  E  slot, page and table ids outside their ranges, under guarded, poisoned memory (both fills): exactly what ref_kvfork says, guards intact;
  F  ``fork`` + ``append`` + ``sageattn_kvcache`` captured into a graph whose replays follow rewritten index arrays and table contents;
  G  draft verification: fork, append 5 draft rows to the fork, attend with Lq 5 bottom-right, append the 3 accepted rows to the original.

Shapes -- the smallest that reach every branch: 8 slots, Hq 8, Hkv 2, D 64 / 128, fp16 / bf16, pages of 64 keys (six per sequence) and of 128
keys (three), a poisoned pool of 32 pages dealt out in a fixed non-ascending order so that the sequences' pages interleave.  Parent lengths
0 / 1 / 63 / 64 (no page; an open tile; a closed tile in an open page with empty tails at 128-key pages, a page boundary at 64-key pages) and
65 / 128 / 130 / 257 (a partial page behind whole ones; page boundaries: no copy).
"""
import functools

import numpy as np
import pytest
import torch

import ref_kvfork
from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi
    from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    DEV = torch.device("cuda:0")

B, HQ, HKV, CAP, ROWS = 8, 8, 2, 384, 512
NUM_PAGES = 32
PAGINGS = [(64, 6), (128, 3)]                      # (page_size, max_pages_per_seq): 384 keys either way
PAGING_IDS = ["page64", "page128"]
PERM = tuple((13 * i + 5) % NUM_PAGES for i in range(NUM_PAGES))      # 5, 18, 31, 12, 25, 6, ...: the order the pool's pages are handed out in
JUNK = (-1, NUM_PAGES, 2 ** 31 - 1)                # what table entries nobody assigned hold, in turn
SETS = [(0, 1, 63, 64), (65, 128, 130, 257)]       # parent lengths
PARENTS, CHILDREN = (5, 0, 6, 3), (1, 7, 2, 4)     # slots, pair by pair
POISON = 0x5A
F16, BF16 = torch.float16, torch.bfloat16
CASES = [(64, F16), (64, BF16), (128, F16), (128, BF16)]
CASE_IDS = ["d64-f16", "d64-bf16", "d128-f16", "d128-bf16"]
BR = dict(is_causal=True, causal_align="bottom_right")
ATTN = [dict(), BR, dict(BR, window_size=(70, 0)), dict(pack_gqa=True), dict(BR, pack_gqa=True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def test_the_page_order_is_a_permutation_that_does_not_ascend():
    assert sorted(PERM) == list(range(NUM_PAGES)) and list(PERM[:4]) != sorted(PERM[:4])


def _ints(values, dtype=torch.int32):
    return torch.tensor(list(values), dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def _content(D, dt):
    """k, v ``[B, HKV, ROWS, D]`` and per-slot frozen statistics (every slot its own): computed once, never modified."""
    g = torch.Generator().manual_seed(31 + D)
    k = (torch.randn(B, HKV, ROWS, D, generator=g) + 1.5 * torch.randn(B, HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = (torch.randn(B, HKV, ROWS, D, generator=g) * (0.25 + torch.rand(B, HKV, 1, D, generator=g))).to(dt).to(DEV)
    km = k[:, :, :257].float().mean(dim=2).to(dt)
    v_amax = v.abs().float().amax(dim=2) * 1.5
    torch.cuda.synchronize()
    return k, v, km, v_amax


def _q(D, dt, lq, seed=3):
    """``[B, HQ, lq, D]``; a child's slot holds its parent's queries"""
    g = torch.Generator().manual_seed(seed + D + lq)
    q = torch.randn(B, HQ, lq, D, generator=g).to(dt).to(DEV)
    q[list(CHILDREN)] = q[list(PARENTS)]
    return q


def _pages_of(n, page_size):
    return (n + page_size - 1) // page_size


def _build(D, dt, paging, parents, fill=POISON, smooth=True):
    """A paged cache whose every byte holds ``fill`` (None: as allocated), seeded slot by slot with the content's statistics, the sequences
    ``parents`` ({slot: length}) filled with the content's first rows through pages dealt round-robin from PERM; every other table entry holds
    JUNK.  Returns (cache, iterator over the pages not yet handed out)."""
    page_size, max_pages = PAGINGS[paging]
    k, v, km, v_amax = _content(D, dt)
    c = PagedQuantizedKVCache.allocate(NUM_PAGES, page_size, B, max_pages, HKV, D, dt, DEV)
    if fill is not None:
        for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail):
            t.view(torch.uint8).fill_(fill)
    pages = iter(PERM)
    rows = [[JUNK[(b * max_pages + e) % 3] for e in range(max_pages)] for b in range(B)]
    for e in range(max_pages):
        for slot, n in parents.items():
            if e < _pages_of(n, page_size):
                rows[slot][e] = next(pages)
    c.block_table.copy_(torch.tensor(rows, dtype=torch.int64).to(torch.int32).to(DEV))
    c.seed(km if smooth else None, v_amax)
    T = max(max(parents.values()), 1)
    c.append(k[:, :, :T], v[:, :, :T], _ints([parents.get(b, 0) for b in range(B)]))
    return c, pages


def _state(c):
    """The cache's tensors as ref_kvfork takes them: integer views on the host (poison and NaN keep their bits)"""
    i = lambda t, dt: t.contiguous().view(dt).cpu().numpy()
    return dict(k_int8=c.k_int8.cpu().numpy(), k_scale=i(c.k_scale, torch.int32), v_image=c.v_image.cpu().numpy(), v_scale=i(c.v_scale, torch.int32),
                v_amax=i(c.v_amax, torch.int32), k_mean=None if c.k_mean is None else i(c.k_mean, torch.int16), k_tail=i(c.k_tail, torch.int16),
                v_tail=i(c.v_tail, torch.int16), lens=c.lens.cpu().numpy(), block_table=c.block_table.cpu().numpy())


def _states_equal(got, want, what):
    for key in ref_kvfork.KEYS:
        if want[key] is None:
            assert got[key] is None, (what, key)
            continue
        diff = got[key] != want[key]
        assert not diff.any(), f"{what}: {key} differs in {int(diff.sum())} elements, first at {[int(a[0]) for a in diff.nonzero()]}"


def _fork_checked(c, src, dst, pages, prefix=None, tensors=None, what="fork"):
    """``c.fork`` of lists (``tensors``: a dtype to hand them over as device tensors of), asserted against ref_kvfork on the state before it.
    Returns (state before, state after)."""
    before = _state(c)
    wrap = (lambda x: x if x is None else list(x)) if tensors is None else (lambda x: x if x is None else _ints(x, tensors))
    c.fork(wrap(src), wrap(dst), wrap(pages), wrap(prefix))
    torch.cuda.synchronize()
    after = _state(c)
    _states_equal(after, ref_kvfork.fork_state(before, c.page_size, src, dst, pages, prefix), what)
    return before, after


def _u8n(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _bits_equal(got, want, what):
    for name, a, b_ in zip(("o", "lse"), got, want):
        ia = a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32)
        ib = b_.contiguous().view(torch.int16 if b_.element_size() == 2 else torch.int32)
        assert a.shape == b_.shape and torch.equal(ia, ib), f"{what}: {name} differs in {int((ia != ib).sum())} of {ia.numel()} elements"


# ---- A: bytes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_a_fork_leaves_exactly_what_the_restatement_says(case, paging):
    D, dt = case
    page_size, max_pages = PAGINGS[paging]
    for lens in SETS:
        parents = dict(zip(PARENTS, lens))
        c, pages = _build(D, dt, paging, parents)
        new = [next(pages) for _ in lens]
        before, after = _fork_checked(c, PARENTS, CHILDREN, new, tensors=torch.int64 if lens is SETS[1] else None, what=f"lens {lens}")
        assert after["lens"][list(CHILDREN)].tolist() == list(lens) and after["lens"][list(PARENTS)].tolist() == list(lens)
        # the parents' slots and pages: bit-identical to the snapshot
        mine = sorted({int(p) for s, n in parents.items() for p in before["block_table"][s][:_pages_of(n, page_size)]})
        for key in ("v_scale", "v_amax", "k_mean", "k_tail", "v_tail", "lens", "block_table"):
            assert (after[key][list(PARENTS)] == before[key][list(PARENTS)]).all(), key
        for key in ("k_int8", "k_scale", "v_image"):
            assert (after[key][mine] == before[key][mine]).all(), key
        # every page that is neither a parent's nor a child's new one still holds the poison, and so does a new page behind what was copied
        rest = sorted(set(range(NUM_PAGES)) - set(mine) - set(new))
        for key in ("k_int8", "k_scale", "v_image"):
            assert (_u8n(after[key][rest]) == POISON).all(), key
        for n, pg in zip(lens, new):
            r = n % page_size
            t = (r + 63) // 64
            assert (_u8n(after["k_int8"][pg, :, 64 * t:]) == POISON).all() and (after["v_image"][pg, :, t:] == POISON).all()
            assert (_u8n(after["k_scale"][pg, :, 4 * t:]) == POISON).all()
            if r:       # ... and what was copied is the parent's open page
                sp = int(before["block_table"][PARENTS[lens.index(n)]][n // page_size])
                assert (after["v_image"][pg, :, :t] == before["v_image"][sp, :, :t]).all() and (after["v_image"][pg, :, :t] != POISON).any()
        # the children's tables: the shared ids, the new page, junk behind
        for s, d, n, pg in zip(PARENTS, CHILDREN, lens, new):
            np_ = n // page_size
            row = after["block_table"][d].tolist()
            assert row[:np_] == before["block_table"][s][:np_].tolist() and row[np_] == pg and row[np_ + 1:] == before["block_table"][d][np_ + 1:].tolist()


def test_a_fork_of_a_cache_without_smoothing():
    c, pages = _build(64, F16, 1, dict(zip(PARENTS, SETS[1])), smooth=False)
    assert c.k_mean is None
    _fork_checked(c, PARENTS, CHILDREN, [next(pages) for _ in PARENTS], tensors=torch.int32)
    assert c.lens.tolist() == [128, 65, 130, 257, 257, 65, 130, 128]


# ---- B: attention -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_b_a_child_attends_as_its_parent(case, paging):
    D, dt = case
    calls = [(lq, kw) for lq in (1, 16) for kw in ATTN]
    for lens in SETS:
        c, pages = _build(D, dt, paging, dict(zip(PARENTS, lens)))
        was = [tuple(t.clone() for t in sageattn_kvcache(_q(D, dt, lq), c, return_lse=True, **kw)) for lq, kw in calls]
        c.fork(list(PARENTS), list(CHILDREN), [next(pages) for _ in lens])
        for (lq, kw), (o0, lse0) in zip(calls, was):
            o, lse = sageattn_kvcache(_q(D, dt, lq), c, return_lse=True, **kw)
            what = f"lens {lens} lq {lq} {kw}"
            _bits_equal((o[list(CHILDREN)], lse[list(CHILDREN)]), (o[list(PARENTS)], lse[list(PARENTS)]), what + ": child against parent")
            _bits_equal((o[list(PARENTS)], lse[list(PARENTS)]), (o0[list(PARENTS)], lse0[list(PARENTS)]), what + ": parent against itself before")
            for s, n in zip(PARENTS, lens):
                assert not bool(torch.isnan(o[s].float()).any())
                if n == 0:
                    assert bool((o[s] == 0).all()) and bool((lse[s] == float("-inf")).all())
                elif not kw.get("is_causal"):         # (a bottom-right row in front of a short parent's first key sees none)
                    assert bool(torch.isfinite(lse[s]).all()) and bool((o[s] != 0).any())


# ---- contiguous references and block-by-block comparison --------------------------------------------------------------------------------
def _contiguous(D, dt, seqs, stats_of):
    """A contiguous cache of capacity CAP whose slot ``b`` holds the rows ``seqs[b]`` = (k ``[HKV, n, D]``, v) under the statistics of slot
    ``stats_of.get(b, b)`` of the content (slots without a sequence: empty)."""
    _, _, km, v_amax = _content(D, dt)
    src = [stats_of.get(b, b) for b in range(B)]
    ref = QuantizedKVCache.allocate(B, HKV, CAP, D, dt, DEV)
    ref.seed(km[src].contiguous(), v_amax[src].contiguous())
    T = max([s[0].shape[1] for s in seqs.values()] + [1])
    k = torch.zeros(B, HKV, T, D, dtype=dt, device=DEV)
    v = torch.zeros(B, HKV, T, D, dtype=dt, device=DEV)
    for b, (kr, vr) in seqs.items():
        k[b, :, :kr.shape[1]], v[b, :, :vr.shape[1]] = kr, vr
    ref.append(k, v, _ints([seqs[b][0].shape[1] if b in seqs else 0 for b in range(B)]))
    return ref


def _same_sequences(c, ref, what):
    """Every slot of the paged cache ``c`` holds, block by block through its table, the bytes of the contiguous cache ``ref``; lengths, V
    scales and the open block's raw rows are equal too."""
    lens = ref.lens.tolist()
    assert c.lens.tolist() == lens, (what, c.lens.tolist(), lens)
    table, tpp = c.block_table.cpu().tolist(), c.page_size // 64
    u8 = lambda t: t.contiguous().view(torch.uint8).cpu()
    pk, ps_, pv = c.k_int8.cpu(), u8(c.k_scale).view(NUM_PAGES, HKV, -1, 16), c.v_image.cpu()
    rk, rs, rv = ref.k_int8.cpu(), u8(ref.k_scale).view(B, HKV, -1, 16), ref.v_image.cpu()
    for b, n in enumerate(lens):
        for j in range((n + 63) // 64):
            page, tip, rows = table[b][j // tpp], j % tpp, min(64, n - 64 * j)
            assert 0 <= page < NUM_PAGES, (what, b, j, page)
            assert torch.equal(pk[page, :, 64 * tip:64 * tip + rows], rk[b, :, 64 * j:64 * j + rows]), f"{what}: slot {b} block {j} (page {page}): INT8 rows"
            assert torch.equal(ps_[page, :, tip], rs[b, :, j]), f"{what}: slot {b} block {j} (page {page}): K scales"
            assert torch.equal(pv[page, :, tip], rv[b, :, j]), f"{what}: slot {b} block {j} (page {page}): V tile"
        assert torch.equal(u8(c.k_tail[b, :, :n % 64]), u8(ref.k_tail[b, :, :n % 64])) and torch.equal(u8(c.v_tail[b, :, :n % 64]), u8(ref.v_tail[b, :, :n % 64])), (what, b)
    assert torch.equal(u8(c.v_scale), u8(ref.v_scale)), what


def _same_attention(c, ref, D, dt, what, calls=((1, dict()), (16, dict(BR, pack_gqa=True)), (16, dict(BR, window_size=(70, 0))))):
    for lq, kw in calls:
        q = _q(D, dt, lq, seed=9)
        _bits_equal(sageattn_kvcache(q, c, return_lse=True, **kw), sageattn_kvcache(q, ref, return_lse=True, **kw), f"{what} lq {lq} {kw}")


def _assign(c, owned, final, pages):
    """Fresh pages into the table entries slot ``b`` needs to grow to ``final[b]`` keys behind the ``owned[b]`` it has"""
    table = c.block_table.cpu()
    for b, n in final.items():
        for e in range(owned[b], _pages_of(n, c.page_size)):
            table[b, e] = next(pages)
    c.block_table.copy_(table.to(DEV))


def _append_rows(c, rows, T):
    """One ``append`` of ``T`` rows: slot ``b`` takes ``rows[b]`` = (k ``[HKV, t, D]``, v), t <= T; every other row holds NaN bits and is not taken"""
    k = torch.full((B, HKV, T, c.D), -1, dtype=torch.int16, device=DEV).view(c.dtype)
    v = k.clone()
    for b, (kr, vr) in rows.items():
        k[b, :, :kr.shape[1]], v[b, :, :vr.shape[1]] = kr, vr
    c.append(k, v, _ints([rows[b][0].shape[1] if b in rows else 0 for b in range(B)]))


# ---- C: divergence ----------------------------------------------------------------------------------------------------------------------
C_STEPS = (1, 63, 2, 64)
C_PARENT = ((1, 63, 2, 64), (1, 0, 2, 64), (0, 63, 0, 0), (1, 0, 2, 64))      # rows pair i's parent takes at each step
C_CHILD = ((0, 63, 2, 0), (1, 63, 0, 64), (1, 63, 2, 64), (1, 63, 2, 0))       # ... and its child


@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_c_parent_and_child_diverge(case, paging):
    D, dt = case
    page_size, max_pages = PAGINGS[paging]
    k, v = _content(D, dt)[:2]
    for lens in SETS:
        c, pages = _build(D, dt, paging, dict(zip(PARENTS, lens)))
        c.fork(list(PARENTS), list(CHILDREN), [next(pages) for _ in lens])
        # slot b's own rows: a child's differ from its parent's behind the fork
        kk, vv = k.clone(), v.clone()
        for s, d, n in zip(PARENTS, CHILDREN, lens):
            kk[d, :, :n], vv[d, :, :n] = k[s, :, :n], v[s, :, :n]
        have = {**dict(zip(PARENTS, lens)), **dict(zip(CHILDREN, lens))}
        counts = {**dict(zip(PARENTS, C_PARENT)), **dict(zip(CHILDREN, C_CHILD))}
        final = {b: have[b] + sum(counts[b]) for b in have}
        assert max(final.values()) <= CAP
        owned = {**{s: _pages_of(n, page_size) for s, n in zip(PARENTS, lens)}, **{d: min(n // page_size + 1, max_pages) for d, n in zip(CHILDREN, lens)}}
        shared = {int(p) for s, n in zip(PARENTS, lens) for p in c.block_table[s, :n // page_size].tolist()}
        _assign(c, owned, final, pages)
        snapshot = [t[sorted(shared)].clone() for t in (c.k_int8, c.k_scale, c.v_image)]
        for i, T in enumerate(C_STEPS):
            _append_rows(c, {b: (kk[b, :, have[b]:have[b] + counts[b][i]], vv[b, :, have[b]:have[b] + counts[b][i]]) for b in have}, T)
            have = {b: have[b] + counts[b][i] for b in have}
        assert have == final
        ref = _contiguous(D, dt, {b: (kk[b, :, :n], vv[b, :, :n]) for b, n in final.items()}, dict(zip(CHILDREN, PARENTS)))
        _same_sequences(c, ref, f"lens {lens}")
        _same_attention(c, ref, D, dt, f"lens {lens}")
        for t, was in zip((c.k_int8, c.k_scale, c.v_image), snapshot):
            assert torch.equal(t[sorted(shared)].view(torch.uint8), was.view(torch.uint8)), "a shared page changed"
        # the two tables share exactly the whole pages of the fork
        table = c.block_table.tolist()
        for s, d, n in zip(PARENTS, CHILDREN, lens):
            np_ = n // page_size
            assert table[s][:np_] == table[d][:np_]
            assert not set(table[s][np_:_pages_of(final[s], page_size)]) & set(table[d][np_:_pages_of(final[d], page_size)])


# ---- D: prefixes ------------------------------------------------------------------------------------------------------------------------
D_PREFIX = (64, 100, 128, 257, 262)
D_CHILDREN = (1, 7, 2, 4, 0)


@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_d_a_prefix_is_the_parents_first_rows(case, paging):
    D, dt = case
    k, v = _content(D, dt)[:2]
    L, s = 257, 5
    c, pages = _build(D, dt, paging, {s: L})
    new = [next(pages) for _ in D_PREFIX]
    _fork_checked(c, [s] * 5, D_CHILDREN, new, D_PREFIX, tensors=torch.int32)
    P = [ref_kvfork.prefix_len(L, w) for w in D_PREFIX]
    assert P == [64, 64, 128, 257, 257] and c.lens.tolist() == [257, 64, 128, 0, 257, 257, 0, 64]
    seqs = {d: (k[s, :, :n], v[s, :, :n]) for d, n in zip(D_CHILDREN, P)}
    seqs[s] = (k[s, :, :L], v[s, :, :L])
    ref = _contiguous(D, dt, seqs, {d: s for d in D_CHILDREN})
    _same_sequences(c, ref, "prefixes")
    _same_attention(c, ref, D, dt, "prefixes")


# ---- E: ids outside their ranges, under the fence ------------------------------------------------------------------------------------------
# D 128, Hkv 2, pages of at most 128 keys, 8 slots: a page (32 KiB at most) or a slot's tails (32 KiB) that an id of -1 or one behind the last
# would name without the checks lies wholly inside the fence's 64 KiB guard -- a missing check fails the comparison or the guard check.
@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
def test_e_ids_outside_their_ranges_write_nothing_they_should_not(paging, fill):
    D, dt = 128, BF16
    page_size, max_pages = PAGINGS[paging]
    assert HKV * page_size * D <= 32 * 1024 and HKV * 64 * D * 2 <= 32 * 1024
    lens = SETS[1]
    with Fence(fill) as f:
        c, pages = _build(D, dt, paging, dict(zip(PARENTS, lens)), fill=None)
        assert all(f.owns(t) for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail, c.lens))
        c.block_table = f.input(c.block_table)
        new = [next(pages) for _ in lens]
        good = (list(PARENTS), list(CHILDREN), new)
        km, v_amax = _content(D, dt)[2:]

        def reset():          # the children as they were before any fork: their own statistics, no rows, new pages that hold the fill
            c.seed(km[list(CHILDREN)].contiguous(), v_amax[list(CHILDREN)].contiguous(), slots=list(CHILDREN))
            for t in (c.k_int8, c.k_scale, c.v_image):
                t.view(torch.uint8)[new] = fill

        for which, bad in ((0, -1), (0, B), (1, -1), (1, B), (2, -1), (2, NUM_PAGES)):
            for i in (0, 3):          # fork 0 (65 keys: an open page to copy) and fork 3 (257 keys: whole pages in front of it)
                reset()
                args = [list(a) for a in good]
                args[which][i] = bad
                before, after = _fork_checked(c, *args, tensors=torch.int32, what=f"argument {which} of fork {i} = {bad}")
                f.check()
                assert (after["v_image"][new[i]] == fill).all() and (after["k_int8"][new[i]].view("uint8") == fill).all()     # nothing went to its page
                if which < 2:         # the fork was skipped: its child is what it was
                    d = CHILDREN[i]
                    assert int(after["lens"][d]) == 0 and all((after[key][d] == before[key][d]).all() for key in ("block_table", "k_tail", "v_amax"))
                else:                 # the table takes the id as given
                    assert int(after["block_table"][CHILDREN[i]][lens[i] // page_size]) == bad and int(after["lens"][CHILDREN[i]]) == lens[i]
                j = 3 - i             # ... and the other fork of the call went through
                assert int(after["lens"][CHILDREN[j]]) == lens[j] and (after["v_image"][new[j], :, 0] != fill).any()
        # an entry of the source's table, where the open page is read
        for i, (s, n) in enumerate(zip(PARENTS, lens)):
            if n % page_size == 0:
                continue
            for bad in (-1, NUM_PAGES):
                reset()
                was = int(c.block_table[s, n // page_size])
                c.block_table[s, n // page_size] = bad
                before, after = _fork_checked(c, *good, tensors=torch.int32, what=f"table[{s}][{n // page_size}] = {bad}")
                f.check()
                assert (after["v_image"][new[i]] == fill).all() and (after["k_int8"][new[i]].view("uint8") == fill).all() and int(after["lens"][CHILDREN[i]]) == n
                c.block_table[s, n // page_size] = was
        reset()
        # ... and all of them good, once more: the children attend as their parents
        _fork_checked(c, *good, tensors=torch.int32, what="all good")
        q = _q(D, dt, 16)
        o, lse = sageattn_kvcache(q, c, return_lse=True, pack_gqa=True, **BR)
        _bits_equal((o[list(CHILDREN)], lse[list(CHILDREN)]), (o[list(PARENTS)], lse[list(PARENTS)]), "under the fence")
        f.check()


# ---- F: graph capture -------------------------------------------------------------------------------------------------------------------
def test_f_fork_append_and_attention_capture_into_a_graph():
    """``fork`` + ``append`` + ``sageattn_kvcache`` captured on one stream; three replays with rewritten ``src_slots`` / ``dst_slots`` /
    ``new_pages``, counts, rows and table contents -- the last one forks a fork -- are bit-equal to the eager sequence, outputs and state."""
    D, dt, paging = 128, BF16, 0
    page_size, max_pages = PAGINGS[paging]
    k, v = _content(D, dt)[:2]
    free = PERM[12:]                                          # (the parents hold 2 + 2 + 3 + 5 pages)

    def fresh():
        c, pages = _build(D, dt, paging, dict(zip(PARENTS, SETS[1])))
        assert next(pages) == free[0]
        return c

    # (src, dst, new pages, the page every later entry of a destination's row names, rows each destination takes)
    steps = [((5, 0), (1, 7), free[0:2], free[2:4], (1, 2)), ((6, 3), (2, 4), free[4:6], free[6:8], (2, 1)), ((1, 5), (2, 4), free[8:10], free[10:12], (2, 2))]
    inputs = []
    for i, (src, dst, new, later, take) in enumerate(steps):
        counts = [0] * B
        for d, t in zip(dst, take):
            counts[d] = t
        inputs.append((_ints(src), _ints(dst), _ints(new), k[:, :, 300 + 2 * i:302 + 2 * i].contiguous(), v[:, :, 300 + 2 * i:302 + 2 * i].contiguous(),
                       _ints(counts), _q(D, dt, 1, seed=20 + i)))

    def rewrite_table(c, i):
        for d, page in zip(steps[i][1], steps[i][3]):
            c.block_table[d] = page

    def step(c, src, dst, new, k_in, v_in, n_in, q_in):
        c.fork(src, dst, new)
        c.append(k_in, v_in, n_in)
        return sageattn_kvcache(q_in, c, pack_gqa=True, return_lse=True, **BR)

    eager_cache, eager = fresh(), []
    for i, s in enumerate(inputs):
        rewrite_table(eager_cache, i)
        eager.append(tuple(t.clone() for t in step(eager_cache, *s)))
    assert eager_cache.lens.tolist() == [128, 66, 68, 257, 67, 65, 130, 130]
    warm, cache = fresh(), fresh()
    static = [t.clone() for t in inputs[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rewrite_table(warm, 0)
        step(warm, *static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o, lse = step(cache, *static)
    for i, s in enumerate(inputs):
        for dst_t, src_t in zip(static, s):
            dst_t.copy_(src_t)
        rewrite_table(cache, i)
        g.replay()
        torch.cuda.synchronize()
        _bits_equal((o, lse), eager[i], f"replay {i}")
    _states_equal(_state(cache), _state(eager_cache), "the replayed cache against the eager one")        # (both pools were poisoned: equal everywhere)


# ---- G: draft verification --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paging", range(len(PAGINGS)), ids=PAGING_IDS)
@pytest.mark.parametrize("case", [(64, BF16), (128, F16)], ids=["d64-bf16", "d128-f16"])
def test_g_draft_rows_are_verified_on_a_fork_and_accepted_into_the_original(case, paging):
    D, dt = case
    page_size, max_pages = PAGINGS[paging]
    k, v = _content(D, dt)[:2]
    lens, n_draft, n_ok = (62, 126, 130, 257), 5, 3       # the draft rows cross a block end (62), a page end (126), neither
    c, pages = _build(D, dt, paging, dict(zip(PARENTS, lens)))
    c.fork(list(PARENTS), list(CHILDREN), [next(pages) for _ in lens])
    owned = {**{s: _pages_of(n, page_size) for s, n in zip(PARENTS, lens)}, **{d: min(n // page_size + 1, max_pages) for d, n in zip(CHILDREN, lens)}}
    _assign(c, owned, {**{s: n + n_ok for s, n in zip(PARENTS, lens)}, **{d: n + n_draft for d, n in zip(CHILDREN, lens)}}, pages)
    draft = {d: (k[d, :, 300:300 + n_draft], v[d, :, 300:300 + n_draft]) for d in CHILDREN}
    _append_rows(c, draft, n_draft)
    prefix = {s: (k[s, :, :n], v[s, :, :n]) for s, n in zip(PARENTS, lens)}
    forked = {d: (torch.cat([prefix[s][0], draft[d][0]], dim=1), torch.cat([prefix[s][1], draft[d][1]], dim=1)) for s, d in zip(PARENTS, CHILDREN)}
    ref1 = _contiguous(D, dt, {**prefix, **forked}, dict(zip(CHILDREN, PARENTS)))
    _same_sequences(c, ref1, "draft rows on the forks")
    _same_attention(c, ref1, D, dt, "verification", calls=((n_draft, BR), (n_draft, dict(BR, pack_gqa=True))))
    _append_rows(c, {s: (draft[d][0][:, :n_ok], draft[d][1][:, :n_ok]) for s, d in zip(PARENTS, CHILDREN)}, n_ok)
    grown = {s: (torch.cat([prefix[s][0], draft[d][0][:, :n_ok]], dim=1), torch.cat([prefix[s][1], draft[d][1][:, :n_ok]], dim=1)) for s, d in zip(PARENTS, CHILDREN)}
    ref2 = _contiguous(D, dt, {**grown, **forked}, dict(zip(CHILDREN, PARENTS)))
    _same_sequences(c, ref2, "accepted rows on the originals")
    _same_attention(c, ref2, D, dt, "after acceptance")
