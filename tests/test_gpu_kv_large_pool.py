"""GPU: the KV-cache family on pools and caches beyond 4 GiB -- pages, K scale slots and V-image tiles at byte offsets of 2^31, 2^32 and more.

Every tile, slot and page address of the cache kernels is a 64-bit product (``k_tile`` / ``v_tile`` / ``ks_slot`` of csrc/sage_attn_body.h, the
append's and the fork's block index, the split's pass 1, the contiguous cache's ``b * k_sb``), and no other test places anything 2 GiB from its
tensor's base: a product that lost its ``(long)`` would pass them all.  Here a ``PagedQuantizedKVCache`` of 4.5 GiB per store tensor
(tests/kv_large_pool_plan.py: geometry (a) D 128, Hkv 8, pages of 256 keys, 18432 pages; (b) D 64, Hkv 2, pages of 64 keys, 589824 pages --
large page INDICES as well) runs a serving program -- a dense append of the prompts, three single-row appends that open a page just past 2^32
bytes, a packed append, three forks (parent's open page high and the children's low and at the very top of the pool; parent low, child high;
a prefix), a last append in which parents and children part -- and every attention route, next to a 64-page TWIN with the same logical table:

  * after every mutating call the per-sequence tensors are equal, every assigned page equals its twin page byte for byte in ``k_int8``,
    ``k_scale`` and ``v_image``, every ALIAS page (4 GiB below an assigned page: where a wrapped 32-bit product lands) still holds the poison --
    asserted on its own, by name -- and a scan of the whole pool in 256 MiB chunks of int64 words finds no word off the poison outside the
    assigned pages;
  * every attention call -- ``sageattn_kvcache`` plain, bottom-right, with a window, with ``pack_gqa``; ``sageattn_kvcache_split`` with S 2, 3
    and "auto", and its workspace through the C entry; ``sageattn_kvcache_varlen``; ``sageattn_kvcache_step`` with both bands -- equals the
    twin's bit for bit;
  * so that a twin wrong in the same way cannot pass, the bottom-right call is held to ``ref_window.attn_window`` on the ledger's operands for
    the longest prompt, a child and the prefix child, at the bars of tests/test_gpu_kvcache_programs.py (2e-3 max|ref| + 2 output ulps, LSE 5e-3).

The contiguous ``QuantizedKVCache`` likewise: B 72 slabs of 64 MiB, keys in slots 2, 31, 32, 63, 64, 65 and 71 (0, 1 and 7 are the aliases of the
last three), a twin of capacity 1536; ``num_splits`` against the big cache's own unsplit call at tests/test_gpu_kv_split.py's bars (the chunk
length follows the capacity, so there is no bit twin).

One big cache lives at a time, inside its test, and is freed there: at most about 10 GiB.  The module skips, saying so, when less than 16 GiB
of device memory is free."""
import traceback

import pytest
import torch

import kv_large_pool_plan as plan
from test_gpu_kv_split import _distance
from test_gpu_paged_kv import _bits_equal
from test_gpu_paged_tile_counts import _anchor_rows, _c_split

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi
    from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    from sageattention_amd.paged_kv_split import sageattn_kvcache_split
    from sageattention_amd.paged_kv_step import sageattn_kvcache_step
    from sageattention_amd.paged_kv_varlen import append_varlen, sageattn_kvcache_varlen
    DEV = torch.device("cuda:0")

GIB = 2 ** 30
POISON = plan.POISON
POISON64 = int.from_bytes(bytes([POISON]) * 8, "little", signed=True)
SCAN_BYTES = 256 * 2 ** 20
NS = plan.NSLOTS
STORE = ("k_int8", "k_scale", "v_image")
PER_SEQUENCE = ("v_scale", "v_amax", "k_mean", "k_tail", "v_tail", "lens")
BR = dict(is_causal=True, causal_align="bottom_right")
VARLEN_Q = (1, 40, 0, 130, 5, 1, 33, 16)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()
    free, total = torch.cuda.mem_get_info()
    print(f"device memory: {free / GIB:.1f} GiB free of {total / GIB:.1f}")
    if free < 16 * GIB:
        pytest.skip(f"the 4 GiB+ pools need 16 GiB of free device memory ({free / GIB:.1f} GiB free): NOT RUN")
    yield
    torch.cuda.empty_cache()


def _ints(values, dtype=torch.int32):
    return torch.tensor([int(x) for x in values], dtype=dtype, device=DEV)


def _u8(t):
    return t.contiguous().view(torch.uint8)


def _poison(c):
    for name in STORE + PER_SEQUENCE[:-1]:
        getattr(c, name).view(torch.uint8).fill_(POISON)


def _dirty(t):
    """The units (pages, slabs) of ``t``'s first dimension that hold an int64 word off the poison: a scan in chunks of at most 256 MiB."""
    n = t.shape[0]
    w = t.view(torch.uint8).view(n, -1).view(torch.int64)
    step = max(1, SCAN_BYTES // (8 * w.shape[1]))
    return set(torch.cat([(w[i:i + step] != POISON64).any(dim=1) for i in range(0, n, step)]).nonzero().flatten().tolist())


def _rows(seed, shape, dt, bias=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) + bias * torch.randn(1, shape[1], 1, shape[3], generator=g)).to(dt).to(DEV)


def _check_state(g, big, twin, written, what):
    """After a mutating call: ``written`` -- the pages the program has written so far."""
    tid, assigned = plan.twin_id(g), set(plan.assigned_pages(g))
    for name in PER_SEQUENCE:
        a, b = getattr(big, name), getattr(twin, name)
        assert torch.equal(_u8(a), _u8(b)), f"{what}: {name} differs from the twin's in {int((_u8(a) != _u8(b)).sum())} bytes"
    # the alias of every assigned page at 2^32 bytes and beyond: where a product that wrapped at 32 bits would have written
    for alias, of in sorted(plan.aliases(g).items()):
        for name in STORE:
            assert bool((_u8(getattr(big, name)[alias]) == POISON).all()), \
                f"{what}: ALIAS page {alias} of {name} -- 4 GiB below assigned page {of} -- was written: a page address wrapped at 32 bits"
    pages = sorted(assigned)
    ib, it = _ints(pages, torch.int64), _ints([tid[p] for p in pages], torch.int64)
    for name in STORE:
        a, b = _u8(getattr(big, name)[ib]).view(len(pages), -1), _u8(getattr(twin, name)[it]).view(len(pages), -1)
        bad = (a != b).sum(1).tolist()
        assert not any(bad), f"{what}: {name} differs from the twin's on pages " + ", ".join(f"{p} (twin {tid[p]}: {n} bytes)" for p, n in zip(pages, bad) if n)
        dirty, dirty_twin = _dirty(getattr(big, name)), _dirty(getattr(twin, name))
        assert dirty <= assigned, f"{what}: {name} was written outside the assigned pages, on pages {sorted(dirty - assigned)[:8]}"
        assert {tid[p] for p in dirty} == dirty_twin, (what, name, sorted(dirty), sorted(dirty_twin))
        assert dirty >= written, f"{what}: {name} of pages {sorted(written - dirty)[:8]} holds no written word"


def _program(g, dt, oracle):
    D, Hkv, ps = g.D, g.Hkv, g.page_size
    max_pages = g.cap // ps
    steps = dict(plan.lens_after(g))
    table_big, table_twin = plan.tables(g)
    _, fork_pages, first_own = plan.placement(g)
    tid = plan.twin_id(g)
    big = PagedQuantizedKVCache.allocate(g.num_pages, ps, NS, max_pages, Hkv, D, dt, DEV)
    twin = PagedQuantizedKVCache.allocate(plan.TWIN_PAGES, ps, NS, max_pages, Hkv, D, dt, DEV)
    assert big.k_int8.numel() == big.v_image.numel() == 4 * GIB + GIB // 2
    for c, t in ((big, table_big), (twin, table_twin)):
        _poison(c)
        c.block_table.copy_(_ints([x for row in t for x in row]).view(NS, -1))
    both = (big, twin)
    # one set of frozen statistics for every slot: the mean of the longest prompt, an abs-max with head-room over everything appended later
    L0 = max(g.contexts)
    k0, v0 = _rows(1, (NS, Hkv, L0, D), dt, 1.5), _rows(2, (NS, Hkv, L0, D), dt) * 0.5
    km = k0[0].float().mean(dim=1).to(dt)[None].expand(NS, Hkv, D).contiguous()
    va = (v0.abs().float().amax(dim=(0, 2)) * 2.0)[None].expand(NS, Hkv, D).contiguous()
    hist = [[] for _ in range(NS)]                       # per slot: the raw rows it was given, in order

    def table_now(b):
        return big.block_table[b].tolist()

    def written():
        lens = big.lens.tolist()
        return {table_now(b)[e] for b in range(NS) for e in range(-(-lens[b] // ps))}

    def dense_append(k, v, counts, what):
        for c in both:
            c.append(k, v, _ints(counts))
        for b, n in enumerate(counts):
            if n:
                hist[b].append((k[b, :, :n], v[b, :, :n]))
        torch.cuda.synchronize()
        assert big.lens.tolist() == list(steps[what]), (what, big.lens.tolist())
        _check_state(g, big, twin, written(), what)

    for c in both:
        c.seed(km, va)
    dense_append(k0, v0, list(g.contexts) + [0] * (NS - 4), "prompts")
    for i in range(plan.SINGLE_ROWS):
        dense_append(_rows(10 + i, (NS, Hkv, 1, D), dt, 1.5), _rows(20 + i, (NS, Hkv, 1, D), dt) * 0.5, [int(b == 2) for b in range(NS)], f"single row {i}")
    assert table_now(2)[1] == g.N32 + 7 and g.N32 + 7 in written()
    # a packed append
    counts = plan.VARLEN_COUNTS
    cu = [sum(counts[:b]) for b in range(NS + 1)]
    kp, vp = _rows(30, (cu[-1] + 2, Hkv, 1, D), dt, 1.5).squeeze(2), (_rows(31, (cu[-1] + 2, Hkv, 1, D), dt) * 0.5).squeeze(2)
    for c in both:
        append_varlen(c, kp, vp, _ints(cu), max(counts))
    for b, n in enumerate(counts):
        if n:
            hist[b].append((kp[cu[b]:cu[b + 1]].transpose(0, 1), vp[cu[b]:cu[b + 1]].transpose(0, 1)))
    torch.cuda.synchronize()
    assert big.lens.tolist() == list(steps["append_varlen"])
    _check_state(g, big, twin, written(), "append_varlen")
    # the forks
    for forks in (plan.FORKS[:2], plan.FORKS[2:3], plan.FORKS[3:]):
        src, dst = [s for s, _ in forks], [d for _, d in forks]
        prefix = [plan.FORK_PREFIX[d] for d in dst] if all(d in plan.FORK_PREFIX for d in dst) else None
        big.fork(src, dst, [fork_pages[d] for d in dst], prefix)
        twin.fork(src, dst, [tid[fork_pages[d]] for d in dst], prefix)
        torch.cuda.synchronize()
        for s, d in forks:
            P = int(big.lens[d])
            rows = (torch.cat([k for k, _ in hist[s]], dim=1)[:, :P], torch.cat([v for _, v in hist[s]], dim=1)[:, :P])
            hist[d] = [rows]
            assert table_now(d)[first_own[d]] == fork_pages[d] and table_now(d)[:first_own[d]] == table_now(s)[:first_own[d]]
        _check_state(g, big, twin, written(), f"fork {src} -> {dst}")
    assert big.lens.tolist() == list(steps["fork"]) and g.num_pages - 1 in written()
    T = max(plan.CHILD_COUNTS)
    dense_append(_rows(40, (NS, Hkv, T, D), dt, 1.5), _rows(41, (NS, Hkv, T, D), dt) * 0.5, plan.CHILD_COUNTS, "children")
    assert written() == set(plan.assigned_pages(g)), sorted(set(plan.assigned_pages(g)) - written())

    # ---- attention: every route, big against twin
    hq, lq = 4 * Hkv, 16
    q = _rows(50, (NS, hq, lq, D), dt)
    lens = big.lens.tolist()
    for name, kw in (("plain", dict()), ("bottom-right", BR), ("window", dict(BR, window_size=(70, 0))), ("pack_gqa", dict(BR, pack_gqa=True))):
        got = sageattn_kvcache(q, big, return_lse=True, **kw)
        _bits_equal(got, sageattn_kvcache(q, twin, return_lse=True, **kw), f"sageattn_kvcache {name}")
        assert bool(torch.isfinite(got[0].float()).all())
        if name == "bottom-right":
            for b in (0, 4, 7):                      # the longest prompt, the child that crossed into pages of its own, the prefix child
                kr, vr = torch.cat([k for k, _ in hist[b]], dim=1), torch.cat([v for _, v in hist[b]], dim=1)
                assert kr.shape[1] == lens[b]
                _anchor_rows(oracle, f"ANCHOR geometry {g.name} bottom-right slot {b} ({lens[b]} keys)", D, dt, g.cap, kr, vr, km[b], va[b], q[b], got[0][b],
                             got[1][b], True, lens[b] - lq, 0)
    for S in (2, 3, "auto"):
        _bits_equal(sageattn_kvcache_split(q, big, S, pack_gqa=True, return_lse=True, **BR),
                    sageattn_kvcache_split(q, twin, S, pack_gqa=True, return_lse=True, **BR), f"sageattn_kvcache_split S {S}")
    starts = (big.lens - lq).to(torch.int32)
    for S, pk in ((2, False), (3, True)):
        out = []
        for c in both:
            ws = torch.full((_cabi.kv_split_ws_bytes(NS, hq, lq, D, S),), 0xA5, dtype=torch.uint8, device=DEV).view(torch.float32)
            out.append(_c_split("paged", q, c, True, starts, S, ws, pk) + (ws,))
        _bits_equal(out[0][:2], out[1][:2], f"the C entry, S {S}")
        assert torch.equal(_u8(out[0][2]), _u8(out[1][2])), f"S {S}: the split workspace differs in {int((_u8(out[0][2]) != _u8(out[1][2])).sum())} bytes"
    cu = [sum(VARLEN_Q[:b]) for b in range(NS + 1)]
    qp = _rows(60, (cu[-1], hq, 1, D), dt).squeeze(2)
    for fn in (sageattn_kvcache_varlen, sageattn_kvcache_step):
        for kw in (dict(), dict(window_size=(70, 0))):
            a, b = fn(qp, big, _ints(cu), max(VARLEN_Q), return_lse=True, **kw), fn(qp, twin, _ints(cu), max(VARLEN_Q), return_lse=True, **kw)
            _bits_equal(a, b, f"{fn.__name__} {kw}")
            assert bool(torch.isfinite(a[0].float()).all())
    _check_state(g, big, twin, written(), "after the attention calls")


@pytest.mark.parametrize("name", ["a", "b"])
def test_a_pool_beyond_4_gib_is_its_64_page_twin(oracle_mod, name):
    g = plan.geometry(name)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    try:
        _program(g, torch.bfloat16 if name == "a" else torch.float16, oracle_mod)
    except BaseException as e:
        traceback.clear_frames(e.__traceback__)          # (the frames hold the 9 GiB cache: release it before the next test allocates its own)
        raise
    finally:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    peak = torch.cuda.max_memory_allocated() / GIB
    print(f"geometry {name}: peak device memory {peak:.2f} GiB")
    assert peak <= 12.0, peak


def test_a_contiguous_cache_beyond_4_gib_is_its_short_twin():
    c = plan.CONTIGUOUS
    B, Hkv, D, dt = c["B"], c["Hkv"], c["D"], torch.bfloat16
    lens_of = c["lens"]
    counts = [lens_of.get(b, 0) for b in range(B)]
    T = max(counts)
    try:
        big = QuantizedKVCache.allocate(B, Hkv, c["cap"], D, dt, DEV)
        twin = QuantizedKVCache.allocate(B, Hkv, c["twin_cap"], D, dt, DEV)
        assert big.k_int8.numel() == big.v_image.numel() == 4 * GIB + GIB // 2
        k, v = _rows(70, (B, Hkv, T, D), dt, 1.5), _rows(71, (B, Hkv, T, D), dt) * 0.5
        km = k[2].float().mean(dim=1).to(dt)[None].expand(B, Hkv, D).contiguous()
        va = (v.abs().float().amax(dim=(0, 2)) * 2.0)[None].expand(B, Hkv, D).contiguous()
        for cache in (big, twin):
            _poison(cache)
            cache.seed(km, va)
            cache.append(k, v, _ints(counts))
        torch.cuda.synchronize()
        assert big.lens.tolist() == twin.lens.tolist() == counts
        for name in PER_SEQUENCE:
            assert torch.equal(_u8(getattr(big, name)), _u8(getattr(twin, name))), name
        for alias, of in sorted(plan.contiguous_aliases().items()):
            for name in STORE:
                assert bool((_u8(getattr(big, name)[alias]) == POISON).all()), \
                    f"ALIAS slot {alias} of {name} -- 4 GiB below slot {of} -- was written: a slot address wrapped at 32 bits"
        for b, n in lens_of.items():
            tiles = -(-n // 64)
            for name, rows in (("k_int8", (slice(None), slice(0, n))), ("k_scale", (slice(None), slice(0, 4 * tiles))), ("v_image", (slice(None), slice(0, tiles)))):
                a, t = _u8(getattr(big, name)[b][rows]), _u8(getattr(twin, name)[b][rows])
                assert torch.equal(a, t), f"slot {b}: {name} differs from the twin's in {int((a != t).sum())} bytes"
        for name in STORE:
            assert _dirty(getattr(big, name)) == set(lens_of), (name, sorted(_dirty(getattr(big, name))))
        hq, lq = 4 * Hkv, 16
        q = _rows(72, (B, hq, lq, D), dt)
        for what, kw in (("plain", dict()), ("bottom-right", BR), ("pack_gqa", dict(BR, pack_gqa=True))):
            got = sageattn_kvcache(q, big, return_lse=True, **kw)
            _bits_equal(got, sageattn_kvcache(q, twin, return_lse=True, **kw), what)
            full = sorted(lens_of)
            # (bottom-right the last row stands on the last key; slot 65 holds one key, so its other rows see none)
            assert bool(torch.isfinite(got[1][full][:, :, -1]).all()) and bool(torch.isneginf(got[1][0]).all())
            if what != "plain":
                for S in (2, 255):               # (255: chunks of 5 tiles, so the slots of 449 and 513 keys span two chunks)
                    elem, rms, lse = _distance(sageattn_kvcache(q, big, num_splits=S, return_lse=True, **kw), got, dt)
                    print(f"contiguous {what} num_splits {S}: element {elem:.3f} rel-RMS {rms:.3f} lse {lse:.3f} of their bars")
                    assert elem <= 1.0 and rms <= 1.0 and lse <= 1.0, (what, S, elem, rms, lse)
        for name in STORE:
            assert _dirty(getattr(big, name)) == set(lens_of), name
    finally:
        big = twin = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
