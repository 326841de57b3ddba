"""A pure-Python model of the paged KV cache's page pool (include/sage_kvpool_gfx950.h), written from the statement of the
arithmetic and not from csrc/sage_page_pool.h: the host twins, the kernels and the sanitizer program are held to it word for word.

State: ``ws`` int32 ``[16 + 2 N + B]`` (hdr, free_stack, refcount, n_owned), ``table`` int32 ``[B, mp]``, ``lens`` int32 ``[B]`` -- numpy
arrays the caller may look at and overwrite (hostile words included).  Also here: the random programs of the CPU and GPU tests, and the
invariants a well-formed state keeps."""
import numpy as np

HDR = 16
I32 = np.int32


def _clamp(x, lo, hi):
    return max(lo, min(hi, int(x)))


def ragged_rows(c0, c1, total, max_rows):
    """csrc/sage_ragged.h's clamp, restated for the model: (first, rows)."""
    t = max(int(total), 0)
    q0 = _clamp(c0, 0, t)
    q1 = t if c1 > t else max(int(c1), q0)
    return q0, min(q1 - q0, max(int(max_rows), 0))


class PoolModel:
    def __init__(self, N, B, ps, mp):
        self.N, self.B, self.ps, self.mp, self.cap = N, B, ps, mp, mp * ps
        self.ws = np.zeros(HDR + 2 * N + B, dtype=I32)
        self.table = np.full((B, mp), -1, dtype=I32)
        self.lens = np.zeros(B, dtype=I32)
        self.init()

    # views into ws
    @property
    def hdr(self):
        return self.ws[:HDR]

    @property
    def stack(self):
        return self.ws[HDR:HDR + self.N]

    @property
    def refc(self):
        return self.ws[HDR + self.N:HDR + 2 * self.N]

    @property
    def owned(self):
        return self.ws[HDR + 2 * self.N:]

    def init(self):
        self.ws[:] = 0
        self.hdr[0] = self.N
        self.stack[:] = np.arange(self.N - 1, -1, -1, dtype=I32)

    def _n_free(self):
        return _clamp(self.hdr[0], 0, self.N)

    def _pop(self, nf, k):
        return _clamp(self.stack[nf - 1 - k], 0, self.N - 1)

    def _close(self, nf, popped, refused, asked):
        since = max(int(self.hdr[3]), 0)
        self.hdr[0] = nf - popped
        self.hdr[1] = refused
        self.hdr[2] = min(asked - nf, 2 ** 31 - 1) if refused and asked > nf else 0
        self.hdr[3] = min(since + refused, 2 ** 31 - 1)

    def rows(self, new_lens=None, T=None, cu=None, total=None, max_new=None):
        if new_lens is not None:
            return [_clamp(x, 0, max(T, 0)) for x in new_lens]
        return [ragged_rows(cu[b], cu[b + 1], total, max_new)[1] for b in range(self.B)]

    def reserve(self, new_lens=None, T=None, cu=None, total=None, max_new=None):
        n = self.rows(new_lens, T, cu, total, max_new)
        nf = self._n_free()
        granted = np.zeros(self.B, dtype=I32)
        asked = popped = refused = 0
        for b in range(self.B):
            L = _clamp(self.lens[b], 0, self.cap)
            want = -(-min(L + n[b], self.cap) // self.ps)
            own = _clamp(self.owned[b], 0, self.mp)
            need = max(0, want - own) if n[b] > 0 else 0
            asked += need
            if need == 0:
                granted[b] = n[b]
            elif asked > nf:
                refused += 1
            else:
                for j in range(need):
                    pg = self._pop(nf, asked - need + j)
                    self.table[b, own + j] = pg
                    self.refc[pg] = 1
                self.owned[b] = want
                popped = asked
                granted[b] = n[b]
        self._close(nf, popped, refused, asked)
        return granted

    def release(self, slots):
        freed = []
        for b in slots:
            if not 0 <= b < self.B:
                continue
            for e in range(_clamp(self.owned[b], 0, self.mp)):
                pg = int(self.table[b, e])
                if 0 <= pg < self.N:
                    if self.refc[pg] == 1:
                        freed.append(pg)
                        self.refc[pg] = 0
                    else:
                        self.refc[pg] = I32((int(self.refc[pg]) - 1 + 2 ** 31) % 2 ** 32 - 2 ** 31)
                self.table[b, e] = -1
            self.owned[b] = 0
            self.lens[b] = 0
        nf = self._n_free()
        for pg in sorted(freed, reverse=True):           # the lowest freed id is handed out next
            if nf < self.N:
                self.stack[nf] = pg
                nf += 1
        self.hdr[0] = nf

    def fork_np(self, s, prefix):
        L = _clamp(self.lens[s], 0, self.cap)
        P = L
        if prefix is not None:
            P = _clamp(prefix, 0, L)
            if P < L:
                P &= ~63
        return P, P // self.ps

    def fork_prepare(self, src, dst, prefix_lens=None):
        n = len(src)
        nf = self._n_free()
        new_pages, dst_eff = np.full(n, -1, dtype=I32), np.full(n, -1, dtype=I32)
        owned0 = self.owned.copy()
        asked = popped = refused = 0
        for i in range(n):
            s, d = int(src[i]), int(dst[i])
            if not (0 <= s < self.B and 0 <= d < self.B) or s == d or owned0[d] != 0:
                refused += 1
                continue
            _, np_ = self.fork_np(s, None if prefix_lens is None else prefix_lens[i])
            need = 1 if np_ < self.mp else 0
            asked += need
            if need and asked > nf:
                refused += 1
                continue
            for e in range(np_):
                pg = int(self.table[s, e])
                if 0 <= pg < self.N:
                    self.refc[pg] += 1
            if need:
                pg = self._pop(nf, asked - 1)
                self.refc[pg] = 1
                new_pages[i] = pg
                popped = asked
            self.owned[d] = np_ + need
            dst_eff[i] = d
        self._close(nf, popped, refused, asked)
        return new_pages, dst_eff

    def apply_fork(self, src, dst_eff, new_pages, prefix_lens=None):
        """What sage_kvfork then does to the table and the lengths (include/sage_kvfork_gfx950.h), for tests without a cache."""
        for i in range(len(src)):
            s, d = int(src[i]), int(dst_eff[i])
            if not (0 <= s < self.B and 0 <= d < self.B) or s == d:
                continue
            P, np_ = self.fork_np(s, None if prefix_lens is None else prefix_lens[i])
            self.table[d, :np_] = self.table[s, :np_]
            if np_ < self.mp:
                self.table[d, np_] = new_pages[i]
            self.lens[d] = P

    def advance(self, granted):
        """What an append of ``granted`` rows does to the lengths (rows past the capacity are dropped)."""
        for b in range(self.B):
            L = _clamp(self.lens[b], 0, self.cap)
            self.lens[b] = L + min(int(granted[b]), self.cap - L)

    def check_invariants(self):
        counts = np.zeros(self.N, dtype=np.int64)
        for b in range(self.B):
            assert 0 <= self.owned[b] <= self.mp, (b, self.owned[b])
            for e in range(self.owned[b]):
                assert 0 <= self.table[b, e] < self.N, (b, e, self.table[b, e])
                counts[self.table[b, e]] += 1
            assert (self.table[b, self.owned[b]:] == -1).all(), (b, self.table[b])
        assert (counts == self.refc).all(), (counts, self.refc)
        nf = int(self.hdr[0])
        assert 0 <= nf <= self.N and sorted(self.stack[:nf].tolist()) == np.flatnonzero(counts == 0).tolist(), (nf, self.stack, counts)


# ---- random serving programs ------------------------------------------------------------------------------------------------------------------
def random_program(seed, steps=14):
    """(N, B, ps, mp, ops): ops of ("reserve_dense", new_lens, T) / ("reserve_packed", cu, total, max_new) / ("release", slots) /
    ("fork", src, dst, prefix or None) / ("init",).  Built by running the model, so that the generator can steer into the corners; ``reached`` is a
    set of the corners this program met."""
    rng = np.random.default_rng(seed)
    B, mp = 6, 8
    ps = int(rng.choice([64, 128]))
    N = int(rng.choice([5, 9, 20, 54]))
    m = PoolModel(N, B, ps, mp)
    ops, reached = [], set()
    edge = [1, 63, 64, 65, ps - 1, ps, ps + 1, 2 * ps, m.cap - 1, m.cap, m.cap + 5]
    for _ in range(steps):
        live = [b for b in range(B) if m.owned[b] > 0]
        empty = [b for b in range(B) if m.owned[b] == 0]
        kind = rng.choice(["dense", "dense", "packed", "packed", "release", "fork", "fork", "init"], p=[.2, .15, .2, .1, .14, .1, .1, .01])
        if kind in ("dense", "packed"):
            n = [int(rng.choice([0, 1, 1, int(rng.choice(edge)), int(rng.integers(1, 3 * ps))])) for _ in range(B)]
            for b in range(B):              # land on an edge now and then
                if n[b] and rng.random() < .3:
                    tgt = int(rng.choice([ps, 2 * ps, 64, m.cap]))
                    if tgt > m.lens[b]:
                        n[b] = tgt - int(m.lens[b])
            if kind == "dense":
                T = max(max(n), 1)
                op = ("reserve_dense", np.array(n, dtype=I32), T)
                g = m.reserve(new_lens=op[1], T=T)
            else:
                cu = np.concatenate([[0], np.cumsum(n)]).astype(I32)
                total, max_new = max(int(cu[-1]), 1), max(max(n), 1)
                op = ("reserve_packed", cu, total, max_new)
                g = m.reserve(cu=cu, total=total, max_new=max_new)
            if m.hdr[1] > 0:
                reached.add("dry")
                ref = [b for b in range(B) if n[b] > 0 and g[b] == 0]
                if any(n[b] > 0 and g[b] > 0 for b in range(ref[0], B)):
                    reached.add("refused_in_the_middle")
            m.advance(g)
            for b in range(B):
                if g[b] and m.lens[b] % 64 == 0:
                    reached.add("block_edge")
                if g[b] and m.lens[b] % ps == 0:
                    reached.add("page_edge")
                if g[b] and m.lens[b] == m.cap:
                    reached.add("capacity_edge")
        elif kind == "release":
            if not live:
                continue
            k = int(rng.integers(1, len(live) + 1))
            slots = [int(s) for s in rng.permutation(live)[:k]]
            if rng.random() < .2:
                slots.append(int(rng.choice([-1, B, B + 7])))
            shared = {int(p) for p in range(N) if m.refc[p] > 1}
            holders = [b for b in slots if 0 <= b < B and shared & set(m.table[b, :m.owned[b]].tolist())]
            if len(holders) >= 2:
                reached.add("two_released_share")
            if len(holders) == 1 and shared:
                reached.add("one_sharer_released_first")
            op = ("release", np.array(slots, dtype=I32))
            m.release(slots)
        elif kind == "fork":
            if not live or not empty:
                continue
            k = int(rng.integers(1, len(empty) + 1))
            dst = [int(d) for d in rng.permutation(empty)[:k]]
            one = int(rng.choice(live))
            src = [one if rng.random() < .6 else int(rng.choice(live)) for _ in dst]
            prefix = None
            if rng.random() < .6:
                prefix = [int(rng.choice([0, 64, ps, 2 * ps, int(m.lens[s]), int(m.lens[s]) - 1, int(rng.integers(0, m.cap + 1))])) for s in src]
            if rng.random() < .15:          # refused whatever the stack holds
                j = int(rng.integers(0, k))
                src[j], dst[j] = [(src[j], src[j]), (-1, dst[j]), (src[j], B), (src[j], int(rng.choice(live)))][int(rng.integers(0, 4))]
            op = ("fork", np.array(src, dtype=I32), np.array(dst, dtype=I32), None if prefix is None else np.array(prefix, dtype=I32))
            pages, eff = m.fork_prepare(op[1], op[2], op[3])
            for i in range(k):
                if eff[i] >= 0:
                    P, np_ = m.fork_np(src[i], None if prefix is None else prefix[i])
                    if P % ps == 0 and P > 0:
                        reached.add("fork_page_edge")
                    if np_ == mp:
                        reached.add("fork_full_table")
            if len({s for s, e in zip(src, eff) if e >= 0}) < sum(1 for e in eff if e >= 0):
                reached.add("several_forks_of_one_source")
            if m.hdr[1] > 0 and m.hdr[2] > 0:
                reached.add("fork_dry")
            m.apply_fork(op[1], eff, pages, op[3])
        else:
            op = ("init",)
            m.init()
            m.table[:] = -1
            m.lens[:] = 0
        ops.append(op)
    return N, B, ps, mp, ops, reached


def run_op(m, op):
    """One op on the model; returns (granted | None, new_pages | None, dst_eff | None).  The table and the lengths follow as the append and the
    fork would move them."""
    if op[0] == "reserve_dense":
        g = m.reserve(new_lens=op[1], T=op[2])
        m.advance(g)
        return g, None, None
    if op[0] == "reserve_packed":
        g = m.reserve(cu=op[1], total=op[2], max_new=op[3])
        m.advance(g)
        return g, None, None
    if op[0] == "release":
        m.release(op[1].tolist())
        return None, None, None
    if op[0] == "fork":
        pages, eff = m.fork_prepare(op[1], op[2], op[3])
        m.apply_fork(op[1], eff, pages, op[3])
        return None, pages, eff
    m.init()
    m.table[:] = -1
    m.lens[:] = 0
    return None, None, None
