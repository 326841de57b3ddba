"""GPU: the device-side page pool of the paged quantised KV cache (``sageattention_amd.paged_kv_pool.PagePool``, ``sage_kvpool_*``).

The pool computes nothing new: it chooses pages.  Every property is an equality --
  A  the kernels leave, after every operation of the CPU tests' first 40 random programs, word for word what tests/ref_page_pool.py leaves:
     the workspace, the table, the lengths, ``granted`` / ``new_pages`` / ``dst_eff``; the invariants hold;
  B  a pool-managed cache, filled through ``pool.append`` and ``pool.append_varlen`` across page boundaries, released in part and filled again
     through recycled pages, attends bit for bit as a contiguous ``QuantizedKVCache`` of the same rows (``sageattn_kvcache``, bottom-right,
     ``pack_gqa`` on and off) and as a hand-tabled ``PagedQuantizedKVCache`` (``sageattn_kvcache_step_listed``); pages never handed out keep
     their poison;
  C  ``pool.fork`` children attend as ``cache.fork`` children of a hand-tabled twin do; counts are 1 + children on shared pages; releasing the
     parent frees its unshared pages alone; releasing the rest returns ``n_free`` to ``num_pages``; a fork into a non-empty destination and a
     fork from a dry pool change nothing but ``hdr``;
  D  a step the pool cannot serve: granted slots take their pages as the model says, refused ones append nothing;
  E  under tests/fence.py (both fills): hostile workspace, table, length and index words -- and a workspace ``init`` never wrote -- leave every
     guard intact and every pool byte outside the pages the tables name unchanged;
  F  ``pool.append`` + the listed step captured in one graph replays across page boundaries as the eager run; a second graph of
     ``release`` + ``fork`` follows rewritten index tensors;
  G  two streams with separate caches beside a competing GEMM end in the model's state.

Shapes: B 6, Hq 8, Hkv 2, D 64 (fp16, 64-key pages) and D 128 (bf16, 128-key pages), 8 pages per sequence, pools of 20 and 54 pages.
"""
import functools

import numpy as np
import pytest
import torch

import ref_page_pool as rpp
from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi_kvpool
    from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    from sageattention_amd.paged_kv_list import sageattn_kvcache_step_listed
    from sageattention_amd.paged_kv_pool import PagePool
    DEV = torch.device("cuda:0")

B, HQ, HKV, MP, ROWS = 6, 8, 2, 8, 1100
N_BIG, N_DRY = 6 * 8 + 6, 20
F16, BF16 = torch.float16, torch.bfloat16
CASES = [(64, F16, 64), (128, BF16, 128)]              # (D, dtype, page_size)
CASE_IDS = ["d64-f16-page64", "d128-bf16-page128"]
POISON = 0x5A
BR = dict(is_causal=True, causal_align="bottom_right")
HOSTILE = [-2 ** 31, -2 ** 31 + 1, -65536, -2, -1, 0, 1, 2, 7, 8, 9, 19, 20, 21, 63, 64, 65, 511, 512, 513, 65536, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi_kvpool.load()


def _ints(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(got, want, what):
    for name, a, b in zip(("o", "lse"), got, want):
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what}: {name} differs in {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements"


@functools.lru_cache(maxsize=None)
def _content(D, dt):
    """k, v ``[B, HKV, ROWS, D]``, the frozen statistics and queries: computed once, never modified."""
    g = torch.Generator().manual_seed(77 + D)
    k = (torch.randn(B, HKV, ROWS, D, generator=g) + 1.5 * torch.randn(B, HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = (torch.randn(B, HKV, ROWS, D, generator=g) * (0.25 + torch.rand(B, HKV, 1, D, generator=g))).to(dt).to(DEV)
    km = k[:, :, :300].float().mean(dim=2).to(dt)
    v_amax = v.abs().float().amax(dim=2) * 1.5
    q = torch.randn(B, HQ, 40, D, generator=g).to(dt).to(DEV)
    torch.cuda.synchronize()
    return k, v, km, v_amax, q


def _paged(D, dt, ps, N, poison=POISON):
    k, v, km, v_amax, _ = _content(D, dt)
    c = PagedQuantizedKVCache.allocate(N, ps, B, MP, HKV, D, dt, DEV)
    if poison is not None:
        for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.k_tail, c.v_tail):
            t.view(torch.uint8).fill_(poison)
    c.seed(km, v_amax)
    return c


def _state(pool):
    torch.cuda.synchronize()
    return pool.ws.cpu().numpy().copy(), pool.cache.block_table.cpu().numpy().copy(), pool.cache.lens.cpu().numpy().copy()


def _assert_model(pool, m, what):
    ws, table, lens = _state(pool)
    assert (ws == m.ws).all(), (what, ws[:16], m.ws[:16], np.flatnonzero(ws != m.ws)[:8])
    assert (table == m.table).all() and (lens == m.lens).all(), (what, table, m.table, lens, m.lens)
    m.check_invariants()


class Seqs:
    """The rows every slot holds, slot by slot, as indices into the content: what a contiguous cache is then filled with."""

    def __init__(self, D, dt):
        self.D, self.dt, self.rows = D, dt, [[] for _ in range(B)]

    def take(self, counts, at):
        """slot b takes the content's rows at[b] .. at[b] + counts[b] - 1"""
        for b, n in enumerate(counts):
            self.rows[b] += list(range(at[b], at[b] + n))

    def tensors(self):
        k, v = _content(self.D, self.dt)[:2]
        T = max(max(len(r) for r in self.rows), 1)
        kk, vv = torch.zeros(B, HKV, T, self.D, dtype=self.dt, device=DEV), torch.zeros(B, HKV, T, self.D, dtype=self.dt, device=DEV)
        for b, r in enumerate(self.rows):
            if r:
                kk[b, :, :len(r)], vv[b, :, :len(r)] = k[b][:, r], v[b][:, r]
        return kk, vv, _ints(len(r) for r in self.rows)

    def contiguous(self):
        _, _, km, v_amax, _ = _content(self.D, self.dt)
        ref = QuantizedKVCache.allocate(B, HKV, MP * 128, self.D, self.dt, DEV)
        ref.seed(km, v_amax)
        ref.append(*self.tensors())
        return ref

    def hand_tabled(self, ps, N):
        c = _paged(self.D, self.dt, ps, N)
        c.block_table.copy_(torch.arange(B * MP, dtype=torch.int32, device=DEV).view(B, MP).flip(0))       # slot b: pages (B - 1 - b) * MP ..
        c.append(*self.tensors())
        return c


# ---- A: the device is the model -----------------------------------------------------------------------------------------------------------------
class DevPool:
    """The device entries over plain tensors, shaped like the CPU tests' HostPool."""

    def __init__(self, N, Bn, ps, mp):
        self.lib = _cabi_kvpool.load()
        self.N, self.B, self.ps, self.mp = N, Bn, ps, mp
        self.ws = torch.full((rpp.HDR + 2 * N + Bn,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        self.table = torch.full((Bn, mp), -1, dtype=torch.int32, device=DEV)
        self.lens = torch.zeros(Bn, dtype=torch.int32, device=DEV)
        self.init()

    def _geom(self):
        return (self.ws.data_ptr(), self.ws.numel() * 4, self.table.data_ptr(), self.mp, self.N, self.ps, self.mp, self.B)

    def _ok(self, rc):
        assert rc == 0, self.lib.sage_last_error()

    def init(self):
        self._ok(self.lib.sage_kvpool_init(self.ws.data_ptr(), self.ws.numel() * 4, self.N, self.B, None))

    def run(self, op):
        p = lambda t: None if t is None else t.data_ptr()
        if op[0] == "reserve_dense":
            n, g = _ints(op[1]), torch.full((self.B,), -7, dtype=torch.int32, device=DEV)
            self._ok(self.lib.sage_kvpool_reserve(*self._geom(), p(self.lens), p(n), int(op[2]), None, 1, 1, p(g), None))
            return g.cpu().numpy(), None, None
        if op[0] == "reserve_packed":
            cu, g = _ints(op[1]), torch.full((self.B,), -7, dtype=torch.int32, device=DEV)
            self._ok(self.lib.sage_kvpool_reserve(*self._geom(), p(self.lens), None, 1, p(cu), int(op[2]), int(op[3]), p(g), None))
            return g.cpu().numpy(), None, None
        if op[0] == "release":
            s = _ints(op[1])
            self._ok(self.lib.sage_kvpool_release(*self._geom(), p(self.lens), p(s), len(op[1]), None))
            return None, None, None
        if op[0] == "fork":
            src, dst, pre = _ints(op[1]), _ints(op[2]), None if op[3] is None else _ints(op[3])
            pages, eff = torch.full((len(op[1]),), -7, dtype=torch.int32, device=DEV), torch.full((len(op[1]),), -7, dtype=torch.int32, device=DEV)
            self._ok(self.lib.sage_kvpool_fork_prepare(*self._geom(), p(self.lens), p(src), p(dst), p(pre), len(op[1]), p(pages), p(eff), None))
            return None, pages.cpu().numpy(), eff.cpu().numpy()
        self.init()
        self.table.fill_(-1)
        self.lens.zero_()
        return None, None, None


def test_a_the_device_equals_the_model_after_every_operation():
    n_ops = 0
    for seed in range(40):
        N, Bn, ps, mp, ops, _ = rpp.random_program(seed)
        m, d = rpp.PoolModel(N, Bn, ps, mp), DevPool(N, Bn, ps, mp)
        after = rpp.PoolModel(N, Bn, ps, mp)         # the append's and sage_kvfork's effect on the lengths and the table, from the device's own answers
        for k, op in enumerate(ops):
            want = rpp.run_op(m, op)
            got = d.run(op)
            after.table, after.lens = d.table.cpu().numpy(), d.lens.cpu().numpy()
            if got[0] is not None:
                after.advance(got[0])
            if op[0] == "fork":
                after.apply_fork(op[1], got[2], got[1], op[3])
            d.table.copy_(torch.from_numpy(after.table)), d.lens.copy_(torch.from_numpy(after.lens))
            for name, a, b in zip(("granted", "new_pages", "dst_eff"), got, want):
                assert (a is None and b is None) or (a == b).all(), (seed, k, op[0], name, a, b)
            ws = d.ws.cpu().numpy()
            assert (ws == m.ws).all(), (seed, k, op[0], ws[:16], m.ws[:16], np.flatnonzero(ws != m.ws)[:8])
            assert (after.table == m.table).all() and (after.lens == m.lens).all(), (seed, k, op[0])
            m.check_invariants()
            n_ops += 1
        m.release(list(range(Bn)))
        d.run(("release", np.arange(Bn, dtype=np.int32)))
        assert (d.ws.cpu().numpy() == m.ws).all() and m.hdr[0] == N and bool((d.table == -1).all()) and bool((d.lens == 0).all()), seed
    assert n_ops >= 400


def test_a_release_compacts_a_pool_of_many_pages_over_every_thread():
    """4000 pages (four ids per thread of the compaction), 1024 slots of 4 pages: the last 24 are refused, odd slots released, then all."""
    N, Bn, ps, mp = 4000, 1024, 64, 4
    m, d = rpp.PoolModel(N, Bn, ps, mp), DevPool(N, Bn, ps, mp)
    n = np.full(Bn, 256, dtype=np.int32)
    n[::7] = 300                                       # (clamped to T = 256)
    for op in (("reserve_dense", n, 256), ("release", np.arange(1, Bn, 2, dtype=np.int32)), ("reserve_dense", n // 2, 256),
               ("release", np.arange(Bn - 1, -1, -1, dtype=np.int32))):
        want, got = rpp.run_op(m, op), d.run(op)
        if got[0] is not None:
            assert (got[0] == want[0]).all()
            d.lens.copy_(torch.from_numpy(m.lens))
        assert (d.ws.cpu().numpy() == m.ws).all() and (d.table.cpu().numpy() == m.table).all(), op[0]
        m.check_invariants()
    assert m.hdr[0] == N and m.hdr[3] > 0


# ---- B: end to end ----------------------------------------------------------------------------------------------------------------------------------
def _attend_all(c, ref, tabled, D, dt, what):
    q = _content(D, dt)[4]
    for lq, kw in ((1, BR), (16, dict(BR, pack_gqa=True)), (40, BR)):
        _same(sageattn_kvcache(q[:, :, :lq], c, return_lse=True, **kw), sageattn_kvcache(q[:, :, :lq], ref, return_lse=True, **kw), f"{what} lq {lq} {kw}")
    counts = (1, 2, 0, 5, 33, 1)
    cu = _ints(np.concatenate([[0], np.cumsum(counts)]))
    qp = torch.cat([q[b, :, :n].transpose(0, 1) for b, n in enumerate(counts)]).contiguous()
    _same(sageattn_kvcache_step_listed(qp, c, cu, 33, return_lse=True), sageattn_kvcache_step_listed(qp, tabled, cu, 33, return_lse=True), f"{what} step")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_b_a_pool_managed_cache_attends_as_a_contiguous_and_a_hand_tabled_one(case):
    D, dt, ps = case
    k, v = _content(D, dt)[:2]
    c = _paged(D, dt, ps, N_BIG)
    pool, m, seqs = PagePool(c), rpp.PoolModel(N_BIG, B, ps, MP), Seqs(D, dt)
    handed = set()

    def dense(counts, at):
        T = max(max(counts), 1)
        kk = torch.stack([k[b, :, at[b]:at[b] + T] for b in range(B)])
        vv = torch.stack([v[b, :, at[b]:at[b] + T] for b in range(B)])
        g = pool.append(kk, vv, None if all(n == T for n in counts) else _ints(counts))
        want = m.reserve(new_lens=np.array(counts, dtype=np.int32), T=T)
        m.advance(want)
        assert g.tolist() == want.tolist() == list(counts)
        seqs.take(counts, at)

    def packed(counts, at):
        kk = torch.cat([k[b, :, at[b]:at[b] + n].transpose(0, 1) for b, n in enumerate(counts)]).contiguous()
        vv = torch.cat([v[b, :, at[b]:at[b] + n].transpose(0, 1) for b, n in enumerate(counts)]).contiguous()
        cu = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        g = pool.append_varlen(kk, vv, _ints(cu), max(counts))
        want = m.reserve(cu=cu, total=int(cu[-1]), max_new=max(counts))
        m.advance(want)
        assert g.tolist() == want.tolist() == list(counts)
        seqs.take(counts, at)

    def look(what):
        _assert_model(pool, m, what)
        handed.update(int(x) for x in m.table.flatten() if x >= 0)

    at = [0] * B
    for fn, counts in ((dense, (130, 64, 1, 0, 200, 65)), (packed, (1, 70, 0, 5, 64, 1)), (dense, (1, 1, 1, 1, 1, 1)), (packed, (63, 1, 126, 59, 0, 200))):
        fn(counts, at)
        at = [a + n for a, n in zip(at, counts)]
        look(f"{fn.__name__} {counts}")
    assert len(handed) == sum(-(-int(n) // ps) for n in m.lens) and m.hdr[3] == 0          # every page once: nothing was released yet
    _attend_all(c, seqs.contiguous(), seqs.hand_tabled(ps, N_BIG), D, dt, "filled")
    # two slots go and come back with other rows, through the pages they gave up (the lowest freed id first)
    pool.release([4, 1])
    m.release([4, 1])
    look("release")
    seqs.rows[1], seqs.rows[4] = [], []
    freed_low = int(m.stack[m.hdr[0] - 1])
    for fn, counts, at2 in ((dense, (0, 129, 0, 0, 65, 0), (0, 700, 0, 0, 800, 0)), (packed, (1, 64, 1, 1, 200, 1), (900, 829, 900, 900, 865, 900))):
        fn(counts, at2)
        look(f"refill {counts}")
    assert int(m.table[1, 0]) == freed_low and freed_low in handed
    _attend_all(c, seqs.contiguous(), seqs.hand_tabled(ps, N_BIG), D, dt, "refilled")
    never = sorted(set(range(N_BIG)) - handed)
    assert never and bool((c.k_int8[never].view(torch.uint8) == POISON).all()) and bool((c.v_image[never] == POISON).all()) and \
        bool((c.k_scale[never].view(torch.uint8) == POISON).all()), "a page the pool never handed out was written"
    assert pool.status() == dict(n_free=int(m.hdr[0]), refused_last=0, pages_short=0, refused_total=0)


# ---- C: forks -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_c_pool_forks_attend_as_cache_forks_and_the_counts_follow(case):
    D, dt, ps = case
    k, v, _, _, q = _content(D, dt)
    c, twin = _paged(D, dt, ps, N_BIG), _paged(D, dt, ps, N_BIG)
    pool, m = PagePool(c), rpp.PoolModel(N_BIG, B, ps, MP)
    n0 = (200, 2 * ps, 0, 0, 0, 0)                     # parent 0 ends inside a page, parent 1 on a page boundary
    g = pool.append(k[:, :, :256], v[:, :, :256], _ints(n0))
    m.advance(m.reserve(new_lens=np.array(n0, dtype=np.int32), T=256))
    twin.block_table.copy_(torch.arange(B * MP, dtype=torch.int32, device=DEV).view(B, MP))
    twin.append(k[:, :, :256], v[:, :, :256], _ints(n0))
    assert g.tolist() == list(n0)
    # three children of parent 0 in one call -- whole, a prefix of one block, a prefix rounded down to 128 -- and parent 1 whole
    src, dst, prefix = [0, 0, 0, 1], [2, 3, 4, 5], [10 ** 6, 64, 191, 10 ** 6]
    eff, pages = pool.fork(src, dst, prefix)
    want_pages, want_eff = m.fork_prepare(src, dst, prefix)
    m.apply_fork(src, want_eff, want_pages, prefix)
    assert eff.tolist() == dst == want_eff.tolist() and pages.tolist() == want_pages.tolist()
    _assert_model(pool, m, "fork")
    twin.fork(src, dst, [B * MP + i for i in range(4)], prefix)
    assert c.lens.tolist() == twin.lens.tolist() == [200, 2 * ps, 200, 64, 128, 2 * ps]
    calls = ((1, BR), (16, dict(BR, pack_gqa=True)))
    outs = []
    for lq, kw in calls:
        outs.append(sageattn_kvcache(q[:, :, :lq], c, return_lse=True, **kw))
        _same(outs[-1], sageattn_kvcache(q[:, :, :lq], twin, return_lse=True, **kw), f"fork children lq {lq}")
    # 1 + children on shared pages
    table, refc = m.table, m.refc
    assert refc[table[0, 0]] == (4 if ps == 64 else 3) and refc[table[1, 0]] == 2 and refc[table[1, 1]] == 2 and refc[table[0, 200 // ps]] == 1
    assert all(refc[p] == 1 for p in want_pages)
    # the parent goes: only its unshared pages are free again, the children attend the same bits
    free0 = int(m.hdr[0])
    unshared = sum(1 for e in range(m.owned[0]) if refc[table[0, e]] == 1)
    pool.release([0])
    m.release([0])
    _assert_model(pool, m, "release parent")
    assert m.hdr[0] == free0 + unshared and 0 < unshared < -(-200 // ps)
    for (lq, kw), before in zip(calls, outs):
        now = sageattn_kvcache(q[:, :, :lq], c, return_lse=True, **kw)
        _same((now[0][1:], now[1][1:]), (before[0][1:], before[1][1:]), f"children after the parent's release lq {lq}")
    # a child appends into its own page and still equals the twin
    one = (0, 0, 70, 1, 0, 3)
    pool.append(k[:, :, 300:370], v[:, :, 300:370], _ints(one))
    m.advance(m.reserve(new_lens=np.array(one, dtype=np.int32), T=70))
    tt = twin.block_table.cpu()
    tt[2, 200 // ps + 1] = B * MP + 5
    twin.block_table.copy_(tt.to(DEV))
    twin.append(k[:, :, 300:370], v[:, :, 300:370], _ints(one))
    _assert_model(pool, m, "children append")
    now, ref = sageattn_kvcache(q[:, :, :16], c, return_lse=True, **BR), sageattn_kvcache(q[:, :, :16], twin, return_lse=True, **BR)
    _same((now[0][1:], now[1][1:]), (ref[0][1:], ref[1][1:]), "children after their appends")
    pool.release(_ints([5, 4, 3, 2, 1]))
    m.release([5, 4, 3, 2, 1])
    _assert_model(pool, m, "release all")
    assert pool.status()["n_free"] == N_BIG and bool((c.block_table == -1).all())


def test_c_a_refused_fork_changes_nothing_but_the_header():
    D, dt, ps = CASES[0]
    k, v = _content(D, dt)[:2]
    c = _paged(D, dt, ps, N_DRY)
    pool, m = PagePool(c), rpp.PoolModel(N_DRY, B, ps, MP)
    n0 = (500, 100, 0, 0, 0, 512)                      # 8 + 2 + 8 pages: two are left
    pool.append(k[:, :, :512], v[:, :, :512], _ints(n0))
    m.advance(m.reserve(new_lens=np.array(n0, dtype=np.int32), T=512))
    _assert_model(pool, m, "prefill")

    def frozen():
        torch.cuda.synchronize()
        return [t.clone() for t in (c.block_table, c.lens, c.k_int8, c.k_scale, c.v_image, c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail, pool.ws[4:])]

    before = frozen()
    # into a non-empty destination, onto itself (as tensors: lists are refused on the host), and three children of which the pool serves two
    eff, pages = pool.fork(_ints([0, 1]), _ints([1, 1]))
    m.fork_prepare([0, 1], [1, 1])
    assert eff.tolist() == [-1, -1] and pages.tolist() == [-1, -1]
    assert all(torch.equal(a, b) for a, b in zip(before, frozen()))
    assert pool.status() == dict(n_free=2, refused_last=2, pages_short=0, refused_total=2)
    eff, pages = pool.fork([0, 0, 5, 0], [2, 3, 1, 4], [64, 500, 512, 128])        # the fork of slot 5 shares all eight pages and needs none -- but slot 1 is not empty
    want_pages, want_eff = m.fork_prepare([0, 0, 5, 0], [2, 3, 1, 4], [64, 500, 512, 128])
    m.apply_fork([0, 0, 5, 0], want_eff, want_pages, [64, 500, 512, 128])
    assert eff.tolist() == want_eff.tolist() == [2, 3, -1, -1] and pages.tolist() == want_pages.tolist()
    _assert_model(pool, m, "dry fork")
    assert pool.status() == dict(n_free=0, refused_last=2, pages_short=1, refused_total=4)
    assert c.lens.tolist() == [500, 100, 64, 500, 0, 512] and bool((c.block_table[4] == -1).all())
    pool.release([1])
    m.release([1])
    eff, pages = pool.fork([5], [1])                    # np == max_pages_per_seq: no page of its own
    want_pages, want_eff = m.fork_prepare([5], [1])
    m.apply_fork([5], want_eff, want_pages)
    assert eff.tolist() == [1] and pages.tolist() == [-1] and int(m.owned[1]) == MP
    _assert_model(pool, m, "full-table fork")
    pool.release(list(range(B)))
    assert pool.status()["n_free"] == N_DRY


# ---- D: refusal -------------------------------------------------------------------------------------------------------------------------------------
def test_d_refused_slots_append_nothing():
    D, dt, ps = CASES[0]
    k, v = _content(D, dt)[:2]
    c = _paged(D, dt, ps, N_DRY)
    pool, m = PagePool(c), rpp.PoolModel(N_DRY, B, ps, MP)
    n0 = (130, 300, 500, 64, 400, 1)                   # 3 + 5 + 8 + 1 pages are served; slot 4 asks for 7 of 3 and is refused, and slot 5 behind it as well
    g = pool.append(k[:, :, :500], v[:, :, :500], _ints(n0))
    want = m.reserve(new_lens=np.array(n0, dtype=np.int32), T=500)
    m.advance(want)
    assert g.tolist() == want.tolist() == [130, 300, 500, 64, 0, 0]
    _assert_model(pool, m, "dry prefill")
    assert pool.status() == dict(n_free=3, refused_last=2, pages_short=5, refused_total=2)
    assert c.lens.tolist() == [130, 300, 500, 64, 0, 0] and bool((c.block_table[4:] == -1).all())
    # the refused slot in the middle: slot 0 asks for 5 of 3 pages; slots 1 and 2 behind it need none and are granted; slot 3 stands on a page
    # boundary and asks for one page -- which is there, but the refused need counts: refused
    torch.cuda.synchronize()
    pool_before = [t.clone() for t in (c.k_int8, c.k_scale, c.v_image)]
    n1 = (400, 1, 12, 1, 0, 0)
    g = pool.append(k[:, :, 500:900], v[:, :, 500:900], _ints(n1))
    want = m.reserve(new_lens=np.array(n1, dtype=np.int32), T=400)
    m.advance(want)
    assert g.tolist() == want.tolist() == [0, 1, 12, 0, 0, 0]
    _assert_model(pool, m, "a refusal in the middle")
    assert pool.status() == dict(n_free=3, refused_last=2, pages_short=3, refused_total=4) and c.lens.tolist() == [130, 301, 512, 64, 0, 0]
    written = {int(p) for b in (1, 2) for p in m.table[b] if p >= 0}
    rest = sorted(set(range(N_DRY)) - written)
    assert rest and all(torch.equal(a[rest], b[rest]) for a, b in zip(pool_before, (c.k_int8, c.k_scale, c.v_image))), "a refused slot's pages were written"
    # the packed form: the refused slot's lens advance, its rows are dropped, granted says so
    cu = np.array([0, 1, 1, 1, 66, 67, 68], dtype=np.int32)
    kk, vv = k[0, :, :68].transpose(0, 1).contiguous(), v[0, :, :68].transpose(0, 1).contiguous()
    g = pool.append_varlen(kk, vv, _ints(cu), 65)
    want = m.reserve(cu=cu, total=68, max_new=65)
    assert g.tolist() == want.tolist() == [1, 0, 0, 65, 1, 0]          # slot 3 takes two of the three pages, slot 4 the last, slot 5 is refused
    ws, table, lens = _state(pool)
    assert (ws == m.ws).all() and (table == m.table).all() and lens.tolist() == [131, 301, 512, 129, 1, 1]          # (the refused slot's length advanced: its row was dropped)
    assert bool((c.block_table[5] == -1).all()) and pool.status() == dict(n_free=0, refused_last=1, pages_short=1, refused_total=5)


# ---- E: the fence -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
@pytest.mark.parametrize("mode", ["never_initialised", "hostile_header_and_owned", "hostile_stack_and_counts", "hostile_table_and_lens"])
def test_e_hostile_words_stay_inside_the_fence(mode, fill):
    D, dt, ps = CASES[0]
    k, v = _content(D, dt)[:2]
    rng = np.random.default_rng(sum(map(ord, mode)) + fill)
    words = lambda n: torch.from_numpy(rng.choice(HOSTILE, size=n).astype(np.int64)).to(torch.int32).to(DEV)
    with Fence(fill) as f:
        c = _paged(D, dt, ps, N_DRY, poison=None)       # (every tensor of the cache and of the pool is a fenced allocation of the package)
        for t in (c.k_int8, c.k_scale, c.v_image):
            t.view(torch.uint8).fill_(fill)
        c.block_table = f.input(c.block_table)          # (allocate fills it through torch.full: the table as a fenced tensor of the caller's)
        pool = PagePool(c, _init=mode != "never_initialised")
        assert f.owns(pool.ws) and f.owns(c.block_table) and f.owns(c.lens)
        N = N_DRY
        touched = set()

        def note():                                     # the pages a table names now: what an append or a fork's copy may write
            ids = c.block_table.flatten()
            touched.update(ids[(ids >= 0) & (ids < N)].tolist())

        for step in range(4):
            if mode == "hostile_header_and_owned":
                pool.hdr.copy_(words(16)), pool.n_owned.copy_(words(B))
            elif mode == "hostile_stack_and_counts":
                pool.free_stack.copy_(words(N)), pool.refcount.copy_(words(N))
            elif mode == "hostile_table_and_lens":
                c.block_table.copy_(words(B * MP).view(B, MP)), c.lens.copy_(words(B))
            table0 = c.block_table.clone()
            note()
            g = pool.append(k[:, :, :130], v[:, :, :130], words(B))
            note()
            cu = f.input(words(B + 1))
            g2 = pool.append_varlen(k[0, :, :70].transpose(0, 1).contiguous(), v[0, :, :70].transpose(0, 1).contiguous(), cu, 70)
            note()
            eff, pages = pool.fork(f.input(words(3)), f.input(words(3)), f.input(words(3)))
            note()
            eff2, pages2 = pool.fork(_ints([0, 0, 1]), _ints([3, 4, 5]))
            note()
            pool.release(f.input(words(4)))
            pool.release(_ints([step, 5 - step]))
            assert all(f.owns(t) for t in (g, g2, eff, pages, eff2, pages2))
            f.check()
            table = c.block_table
            changed = table != table0
            assert bool(((table[changed] >= -1) & (table[changed] < N)).all()), "a table entry written by the pool is no page"
            assert bool(((pool.hdr[0] >= 0) & (pool.hdr[0] <= N)).all())
            assert bool(((g >= 0) & (g <= 130)).all()) and bool(((g2 >= 0) & (g2 <= 70)).all())
            assert bool(((pages >= -1) & (pages < N)).all()) and bool(((eff >= -1) & (eff < B)).all()) and bool(((pages2 >= -1) & (pages2 < N)).all())
            rest = sorted(set(range(N)) - touched)
            assert all(bool((t[rest].view(torch.uint8) == fill).all()) for t in (c.k_int8, c.k_scale, c.v_image)), "a page no table named was written"
        f.check()


# ---- F: graphs ------------------------------------------------------------------------------------------------------------------------------------------
def test_f_a_captured_step_replays_across_page_boundaries():
    D, dt, ps = CASES[0]
    k, v, _, _, q = _content(D, dt)
    n0 = (63, 62, 61, 1, 0, 130)
    cu = _ints(range(B + 1))

    def fresh():
        c = _paged(D, dt, ps, N_BIG)
        pool = PagePool(c)                              # (init runs outside the graph)
        pool.append(k[:, :, :130], v[:, :, :130], _ints(n0))
        return pool

    def step(pool, k_in, v_in, q_in):
        g = pool.append(k_in, v_in)
        return (g,) + tuple(sageattn_kvcache_step_listed(q_in, pool.cache, cu, 1, return_lse=True))

    steps = [(k[:, :, 200 + i:201 + i].contiguous(), v[:, :, 200 + i:201 + i].contiguous(), q[:, :, i].contiguous()) for i in range(5)]
    eager_pool, eager = fresh(), []
    for s in steps:
        out = step(eager_pool, *s)
        eager.append(tuple(t.clone() for t in out) + _state(eager_pool))
    crossed = [sum(1 for b in range(B) if -(-(n0[b] + i + 1) // ps) > -(-(n0[b] + i) // ps)) for i in range(5)]
    assert sum(1 for x in crossed if x) >= 3, crossed

    warm, pool = fresh(), fresh()
    k_in, v_in, q_in = (t.clone() for t in steps[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(warm, k_in, v_in, q_in)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(pool, k_in, v_in, q_in)
    for i, s in enumerate(steps):
        k_in.copy_(s[0]), v_in.copy_(s[1]), q_in.copy_(s[2])
        graph.replay()
        ws, table, lens = _state(pool)
        for name, a, b in zip(("granted", "o", "lse"), out, eager[i][:3]):
            assert torch.equal(_bits(a), _bits(b)), f"replay {i}: {name}"
        assert (ws == eager[i][3]).all() and (table == eager[i][4]).all() and (lens == eager[i][5]).all(), f"replay {i}"
    assert pool.cache.lens.tolist() == [n + 5 for n in n0]


def test_f_release_and_fork_replay_with_rewritten_index_tensors():
    D, dt, ps = CASES[0]
    k, v, _, _, q = _content(D, dt)
    n0 = (200, 128, 65, 0, 0, 0)

    def fresh():
        c = _paged(D, dt, ps, N_BIG)
        pool = PagePool(c)
        pool.append(k[:, :, :200], v[:, :, :200], _ints(n0))
        return pool

    def step(pool, slots, src, dst, prefix):
        pool.release(slots)
        return pool.fork(src, dst, prefix)

    rounds = [([3, 4], [0, 1], [3, 4], [128, 500]), ([4, 0], [1, 2], [0, 4], [64, 65]), ([5, 3], [0, 2], [5, 3], [1, 0])]
    eager_pool, m, eager = fresh(), rpp.PoolModel(N_BIG, B, ps, MP), []
    m.advance(m.reserve(new_lens=np.array(n0, dtype=np.int32), T=200))
    for r in rounds:
        out = step(eager_pool, *(_ints(x) for x in r))
        m.release(r[0])
        pages, eff = m.fork_prepare(r[1], r[2], r[3])
        m.apply_fork(r[1], eff, pages, r[3])
        _assert_model(eager_pool, m, f"eager {r}")
        assert out[0].tolist() == eff.tolist() and out[1].tolist() == pages.tolist()
        eager.append((out[0].clone(), out[1].clone()) + _state(eager_pool) + tuple(sageattn_kvcache(q[:, :, :1], eager_pool.cache, return_lse=True)))
    warm, pool = fresh(), fresh()
    ins = [_ints(x) for x in rounds[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(warm, *ins)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(pool, *ins)
    for i, r in enumerate(rounds):
        for t, x in zip(ins, r):
            t.copy_(_ints(x))
        graph.replay()
        ws, table, lens = _state(pool)
        assert torch.equal(out[0], eager[i][0]) and torch.equal(out[1], eager[i][1]), f"replay {i}"
        assert (ws == eager[i][2]).all() and (table == eager[i][3]).all() and (lens == eager[i][4]).all(), f"replay {i}"
        _same(sageattn_kvcache(q[:, :, :1], pool.cache, return_lse=True), eager[i][5:], f"replay {i}")


# ---- G: streams ---------------------------------------------------------------------------------------------------------------------------------------
def test_g_two_streams_with_their_own_pools_beside_a_gemm():
    D, dt, ps = CASES[0]
    k, v, _, _, q = _content(D, dt)
    n0 = (60, 1, 127, 0, 300, 500)
    cu = _ints(range(B + 1))
    iters = 36
    pools = []
    for _ in range(2):
        c = _paged(D, dt, ps, N_DRY)                    # 20 pages: 17 at the start, three more on the way, and slot 4 is refused from 320 keys on
        pool = PagePool(c)
        pool.append(k[:, :, :500], v[:, :, :500], _ints(n0))
        pools.append(pool)
    m = rpp.PoolModel(N_DRY, B, ps, MP)
    m.advance(m.reserve(new_lens=np.array(n0, dtype=np.int32), T=500))
    outs = [[], []]
    a = torch.randn(1024, 1024, device=DEV, dtype=torch.float16)
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for i in range(iters):
        for j in (0, 1):
            with torch.cuda.stream(streams[j]):
                pools[j].append(k[:, :, 600 + i:601 + i], v[:, :, 600 + i:601 + i])
                outs[j].append(sageattn_kvcache_step_listed(q[:, :, i % 40].contiguous(), pools[j].cache, cu, 1, return_lse=True))
        with torch.cuda.stream(streams[2]):
            a = (a @ a).clamp_(-1, 1)
        m.advance(m.reserve(new_lens=np.ones(B, dtype=np.int32), T=1))
    torch.cuda.synchronize()
    assert m.hdr[3] > 0 and m.hdr[0] == 0, m.hdr[:4]
    for j in (0, 1):
        _assert_model(pools[j], m, f"stream {j}")
    for x, y in zip(outs[0], outs[1]):
        _same(x, y, "the two streams")
