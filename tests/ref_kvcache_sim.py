"""A page-free model of the quantised KV-cache family and a byte-level restatement of its kernels' write sets -- TEST INFRASTRUCTURE ONLY.

Two layers that check each other (tests/test_kvcache_sim_host.py on the CPU; tests/test_gpu_kvcache_programs.py holds the GPU to both):

``Ledger`` is the DEFINITION.  It knows nothing of pages, blocks kept open, tails or tables: per slot it records the raw fp16 / bf16 rows appended
so far (bit patterns) and the slot's frozen ``k_mean`` / ``v_amax``, and derives the operands an attention call is entitled to read:
  K8, k_scale  per 64-row block, per-thread K groups (row r of a block: group ``(r % 8) // 2``), the mean subtracted and rounded to the input
               dtype, ``scale = amax / 127 + 1e-7``: ``oracle.quant_int8(style=STYLE_TRITON_THREAD, mean=)`` on the block's valid rows;
  V8           ``e4m3(clamp(x * fp32(448 / v_amax), -448, 448))`` rounded to nearest even, written here from the format alone (1-4-3 bits,
               bias 7, subnormal unit 2^-9, largest finite value 448 = 0x7e); a channel with ``v_amax == 0`` holds zeros;
  v_scale      ``v_amax / 448`` in fp32.

The SIMULATOR restates what ``sage_kvcache_append`` / ``sage_kvpaged_append`` / ``sage_kvpvarlen_append`` / ``sage_kvfork`` and ``seed`` leave behind,
byte by byte, on the state layout of tests/ref_kvfork.py (a dict of ten arrays, ``KEYS``; integer views, so poison keeps its bits):
  * ``seed`` writes the statistics rows (``k_mean``, ``v_amax``) of the named slots and zeroes their ``lens`` -- nothing else: ``v_scale``, the
    tails, the table and the pool keep what they hold;
  * an append gives slot b ``t = min(clamp(count, 0, T), capacity - clamp(lens[b], 0, capacity))`` rows (packed: ``count = min(cu[b + 1] - cu[b],
    max_new)``); every 64-row block that gains a row is re-formed from the tails plus the new rows: its K rows ``< valid``, its four scale
    slots, its whole V tile (zeros behind ``valid``); ``v_scale`` of EVERY slot is written on every call; the tails take rows ``lo .. len1 - 1`` of
    the open block (``lo = max(len0, len1 // 64 * 64)``), nothing when the append ends on a block boundary; ``lens`` is written (clamped); a
    block whose table entry lies outside the pool writes nothing while ``lens`` still advances; no other byte changes;
  * a fork is ``ref_kvfork.fork_state``, as it is.
A contiguous ``QuantizedKVCache`` is the same state with one page of ``capacity`` keys per slot and the identity table.

``logical(state, page_size, b)`` gathers slot b's first ``lens[b]`` keys through the table; ``logical_mismatches`` holds that against the ledger,
``state_mismatches`` holds one state against another and names tensor, slot or page.  ``random_program(seed)`` draws a shape and 10 - 14
operations (pure Python, its own random stream, an allocator with reference counts included); ``Run`` turns a program's steps into concrete
arrays and keeps ledger and simulator in step.  Nothing here imports ``sageattention_amd``.
"""
from __future__ import annotations

import random

import numpy as np

import util
from ref_kvfork import KEYS, fork_state, prefix_len

NSLOTS, HKV, CAP = 6, 2, 512
PAGE_SIZES = (64, 128, 256)
SPARE_PAGES = 6                   # pages of the pool beyond what six full slots need
POISON = 0x5A
HEADROOMS = (1.0, 1.5, 2.0)
DENSE_LQS = (1, 16, 40, 130)
VARLEN_LQS = (0, 1, 5, 17, 64, 129, 130)
SPLITS = (2, 3, 8)
MUTATING = ("prefill", "append", "append_varlen", "fork", "reseed")
ROUTES = ("dense_nc", "dense_tl", "dense_br", "dense_qstart", "dense_window", "dense_pack", "split", "varlen", "varlen_window", "varlen_qstart")
MUTANTS = ("fork_shares_open_page", "stale_k_scale", "v_content_amax", "table_half_page", "reseed_keeps_v_amax")


# ---------------------------------------------------------------------------------------------------------------- number formats
def to_bits(x: np.ndarray, code: int) -> np.ndarray:
    """fp32 -> fp16 (code 0) / bf16 (code 1) bit patterns, round to nearest even (finite values)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if code == 0:
        return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def e4m3_rne(x: np.ndarray) -> np.ndarray:
    """fp32 -> OCP e4m3fn bytes, round to nearest even, saturating at +-448 -- from the format: sign, 4 exponent bits of bias 7, 3 mantissa
    bits; exponent field 0 is subnormal with unit 2^-9; there is no infinity and 0x7e = 448 is the largest finite value.  A value with
    leading-bit exponent ``E >= -6`` is ``q * 2^(E - 3)`` with ``q`` in [8, 16) and has the code ``8 * (E + 7) + q - 8``; the subnormals share
    ``E = -6`` with ``q`` in [0, 8) and the same expression gives their code ``q``; a mantissa that rounds up to 16 carries into the exponent by
    the same arithmetic.  Finite inputs only."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    a = np.minimum(np.abs(x), np.float32(448.0))
    _, e = np.frexp(a)                                            # a = m * 2^e with m in [0.5, 1): leading bit at e - 1
    E = np.where(a > 0, np.maximum(e - 1, -6), -6).astype(np.int32)
    q = np.rint(np.ldexp(a, 3 - E)).astype(np.int32)              # exact scaling by a power of two, then round half to even
    code = 8 * (E + 7) + q - 8
    assert int(code.min(initial=0)) >= 0 and int(code.max(initial=0)) <= 0x7E
    return (code.astype(np.uint8) | (np.signbit(x).astype(np.uint8) << 7)).astype(np.uint8)


def quant_v_rows(v_bits: np.ndarray, v_amax: np.ndarray, code: int) -> np.ndarray:
    """V8 of rows ``[H, n, D]`` under the frozen abs-max ``v_amax`` fp32 ``[H, D]``: ``x * fp32(448 / v_amax)``, clamped, to e4m3; zeros where
    ``v_amax == 0``."""
    am = np.ascontiguousarray(v_amax, dtype=np.float32)[:, None, :]
    with np.errstate(divide="ignore"):
        recp = np.where(am > 0, np.float32(448.0) / am, np.float32(0.0)).astype(np.float32)
    y = util.f32(np.ascontiguousarray(v_bits), code) * recp
    out = e4m3_rne(np.clip(y, np.float32(-448.0), np.float32(448.0)))
    return np.where(am > 0, out, np.uint8(0)).astype(np.uint8)


def v_scale_of(v_amax: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(v_amax, dtype=np.float32) / np.float32(448.0)).astype(np.float32)


def quant_k_block(oracle, k_bits: np.ndarray, k_mean, code: int):
    """(K8 int8 [H, n, D], k_scale fp32 [H, 4]) of the ``n <= 64`` valid rows of one block: the oracle's quantiser with the per-thread K groups
    of a 64-key block; a group without a valid row gets the scale 1e-7."""
    n = k_bits.shape[1]
    assert 1 <= n <= 64
    grp, ng = oracle.group_index(n, "per_thread", "k", 64, 64)
    assert ng == 4
    mean = None if k_mean is None else np.ascontiguousarray(k_mean, dtype=np.uint16)[None]
    k8, ks = oracle.quant_int8(np.ascontiguousarray(k_bits, dtype=np.uint16)[None], code, grp, 4, style=oracle.STYLE_TRITON_THREAD, mean=mean)
    return k8[0], ks[0]


# ---------------------------------------------------------------------------------------------------------------- the ledger
class Ledger:
    """The definition: per slot the raw rows and the frozen statistics; ``operands(b)`` derives what attention may read."""

    def __init__(self, oracle, nslots, H, D, code, cap):
        self.oracle, self.H, self.D, self.code, self.cap = oracle, H, D, code, cap
        self.k = [np.zeros((H, 0, D), np.uint16) for _ in range(nslots)]
        self.v = [np.zeros((H, 0, D), np.uint16) for _ in range(nslots)]
        self.k_mean = [None] * nslots              # uint16 [H, D] or None
        self.v_amax = [None] * nslots              # fp32 [H, D]
        self._closed = [[] for _ in range(nslots)]     # derived closed blocks, kept: (K8, k_scale, V8) each

    def length(self, b):
        return self.k[b].shape[1]

    def seed(self, slots, k_mean, v_amax):
        for i, b in enumerate(slots):
            self.k_mean[b] = None if k_mean is None else np.array(k_mean[i], dtype=np.uint16)
            self.v_amax[b] = np.array(v_amax[i], dtype=np.float32)
            self.k[b], self.v[b], self._closed[b] = self.k[b][:, :0], self.v[b][:, :0], []

    def append(self, b, k_rows, v_rows):
        """Rows ``[H, n, D]``; what does not fit into the capacity is dropped."""
        n = min(k_rows.shape[1], self.cap - self.length(b))
        if n > 0:
            self.k[b] = np.concatenate((self.k[b], k_rows[:, :n]), axis=1)
            self.v[b] = np.concatenate((self.v[b], v_rows[:, :n]), axis=1)

    def fork(self, src, dst, prefix=None):
        """The child holds the parent's first P rows (a prefix shorter than the parent: rounded down to a multiple of 64) and its statistics."""
        P = prefix_len(self.length(src), prefix)
        self.k[dst], self.v[dst] = self.k[src][:, :P].copy(), self.v[src][:, :P].copy()
        self.k_mean[dst] = None if self.k_mean[src] is None else self.k_mean[src].copy()
        self.v_amax[dst] = self.v_amax[src].copy()
        self._closed[dst] = list(self._closed[src][:P // 64])

    def _block(self, b, i):
        rows = slice(64 * i, min(64 * i + 64, self.length(b)))
        k8, ks = quant_k_block(self.oracle, self.k[b][:, rows], self.k_mean[b], self.code)
        return k8, ks, quant_v_rows(self.v[b][:, rows], self.v_amax[b], self.code)

    def operands(self, b):
        """K8 int8 [H, L, D], k_scale fp32 [H, 4 * ceil(L / 64)], V8 uint8 [H, L, D], v_scale fp32 [H, D] of slot b's L rows."""
        L = self.length(b)
        closed = self._closed[b]
        del closed[L // 64:]
        while len(closed) < L // 64:
            closed.append(self._block(b, len(closed)))
        blocks = closed + ([self._block(b, L // 64)] if L % 64 else [])
        H, D = self.H, self.D
        cat = lambda j, empty: np.concatenate([blk[j] for blk in blocks], axis=1) if blocks else empty
        return dict(K8=cat(0, np.zeros((H, 0, D), np.int8)), k_scale=cat(1, np.zeros((H, 0), np.float32)), V8=cat(2, np.zeros((H, 0, D), np.uint8)),
                    v_scale=v_scale_of(self.v_amax[b]))


# ---------------------------------------------------------------------------------------------------------------- the simulator
def poisoned_state(num_pages, page_size, nslots, max_pages, H, D, smooth, table):
    """The ten arrays of a cache whose every byte holds POISON, ``lens`` zero, the table as given."""
    p16, p32 = np.int16(POISON * 0x0101), np.int32(POISON * 0x01010101)
    return dict(k_int8=np.full((num_pages, H, page_size, D), POISON, np.int8), k_scale=np.full((num_pages, H, page_size // 64 * 4), p32, np.int32),
                v_image=np.full((num_pages, H, page_size // 64, D, 64), POISON, np.uint8), v_scale=np.full((nslots, H, D), p32, np.int32),
                v_amax=np.full((nslots, H, D), p32, np.int32), k_mean=np.full((nslots, H, D), p16, np.int16) if smooth else None,
                k_tail=np.full((nslots, H, 64, D), p16, np.int16), v_tail=np.full((nslots, H, 64, D), p16, np.int16),
                lens=np.zeros((nslots,), np.int32), block_table=np.array(table, dtype=np.int32).reshape(nslots, max_pages))


def _f32_of(a):
    return np.ascontiguousarray(a).view(np.float32)


class Simulator:
    """The kernels' write sets on a state dict.  ``mutant``: one of MUTANTS, a deliberately wrong cache for tests/test_kvcache_sim_host.py."""

    def __init__(self, oracle, page_size, code, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.oracle, self.page_size, self.code, self.mutant = oracle, page_size, code, mutant
        self.shift = (page_size // 64).bit_length() - 1
        assert page_size == 64 << self.shift

    def seed(self, state, slots, k_mean, v_amax):
        slots = list(slots)
        if (k_mean is None) != (state["k_mean"] is None):
            raise ValueError("smoothing is one choice for every slot of a cache")
        if k_mean is not None:
            state["k_mean"][slots] = np.ascontiguousarray(k_mean, dtype=np.uint16).view(np.int16)
        if self.mutant != "reseed_keeps_v_amax" or bool((state["v_amax"][slots] == np.int32(POISON * 0x01010101)).all()):
            state["v_amax"][slots] = np.ascontiguousarray(v_amax, dtype=np.float32).view(np.int32)
        state["lens"][slots] = 0

    def append(self, state, k_rows, v_rows, new_lens=None):
        """Dense rows ``[B, H, T, D]`` (bit patterns); ``new_lens`` ints or None (all T)."""
        T = k_rows.shape[2]
        counts = [T if new_lens is None else max(0, min(int(n), T)) for n in (new_lens if new_lens is not None else [T] * k_rows.shape[0])]
        self._append(state, counts, lambda b: (k_rows[b], v_rows[b]))

    def append_varlen(self, state, k_packed, v_packed, cu, max_new):
        """Packed rows ``[total, H, D]``; slot b takes the first ``min(cu[b + 1] - cu[b], max_new)`` rows of its stretch."""
        cu = [int(x) for x in cu]
        counts = [max(0, min(cu[b + 1] - cu[b], int(max_new))) for b in range(len(cu) - 1)]
        take = lambda b: (np.swapaxes(k_packed[cu[b]:cu[b] + counts[b]], 0, 1), np.swapaxes(v_packed[cu[b]:cu[b] + counts[b]], 0, 1))
        self._append(state, counts, take)

    def fork(self, state, src, dst, pages, prefix=None):
        out = fork_state(state, self.page_size, src, dst, pages, prefix)
        if self.mutant == "fork_shares_open_page":
            for s, d in zip(src, dst):
                P = int(out["lens"][d])
                if P % self.page_size:
                    out["block_table"][d, P // self.page_size] = state["block_table"][s, P // self.page_size]
        for key in KEYS:
            if state[key] is not None:
                state[key][...] = out[key]

    def _append(self, state, counts, rows_of):
        ps, shift, code = self.page_size, self.shift, self.code
        num_pages, nslots, cap = state["k_int8"].shape[0], state["lens"].shape[0], state["block_table"].shape[1] * self.page_size
        v_amax = _f32_of(state["v_amax"])
        state["v_scale"][...] = v_scale_of(v_amax).view(np.int32)                       # every slot, every call
        for b in range(nslots):
            len0 = min(max(int(state["lens"][b]), 0), cap)
            t = min(counts[b], cap - len0)
            len1 = len0 + t
            k_new, v_new = rows_of(b)
            mean = None if state["k_mean"] is None else state["k_mean"][b].view(np.uint16)
            for blk in range(len0 // 64, (len1 + 63) // 64 if t > 0 else 0):
                row0 = 64 * blk
                if row0 >= len1:
                    continue
                valid, old = min(len1 - row0, 64), max(len0 - row0, 0)
                entry, at = blk >> shift, blk & ((1 << shift) - 1)
                if self.mutant == "table_half_page" and shift > 0 and at >= (1 << shift) // 2:
                    entry = blk >> (shift + 1)
                page = int(state["block_table"][b, entry])
                if not 0 <= page < num_pages:
                    continue
                new = slice(row0 + old - len0, row0 + valid - len0)
                kb = np.concatenate((state["k_tail"][b, :, :old].view(np.uint16), k_new[:, new]), axis=1)
                vb = np.concatenate((state["v_tail"][b, :, :old].view(np.uint16), v_new[:, new]), axis=1)
                k8, ks = quant_k_block(self.oracle, kb, mean, code)
                state["k_int8"][page, :, 64 * at:64 * at + valid] = k8
                if not (self.mutant == "stale_k_scale" and old > 0):
                    state["k_scale"][page, :, 4 * at:4 * at + 4] = ks.view(np.int32)
                am = v_amax[b]
                if self.mutant == "v_content_amax":
                    am = np.abs(util.f32(np.ascontiguousarray(vb), code)).max(axis=1)
                tile = np.zeros((vb.shape[0], 64, vb.shape[2]), np.uint8)
                tile[:, :valid] = quant_v_rows(vb, am, code)
                state["v_image"][page, :, at] = util.encode_v_image(tile, True)[:, 0]
            open0 = len1 // 64 * 64
            lo = max(len0, open0)
            n = len1 - lo
            if n > 0:
                state["k_tail"][b, :, lo - open0:lo - open0 + n] = np.ascontiguousarray(k_new[:, lo - len0:lo - len0 + n]).view(np.int16)
                state["v_tail"][b, :, lo - open0:lo - open0 + n] = np.ascontiguousarray(v_new[:, lo - len0:lo - len0 + n]).view(np.int16)
            state["lens"][b] = len1


def logical(state, page_size, b):
    """Slot b's first ``lens[b]`` keys gathered through the table: K8, k_scale (fp32), V8 (decoded from the tile image), v_scale (fp32)."""
    shift = (page_size // 64).bit_length() - 1
    num_pages = state["k_int8"].shape[0]
    L = int(state["lens"][b])
    H, D = state["k_int8"].shape[1], state["k_int8"].shape[3]
    k8, ks, v8 = [np.zeros((H, 0, D), np.int8)], [np.zeros((H, 0), np.float32)], [np.zeros((H, 0, D), np.uint8)]
    for blk in range((L + 63) // 64):
        page, at = int(state["block_table"][b, blk >> shift]), blk & ((1 << shift) - 1)
        assert 0 <= page < num_pages, f"slot {b}: logical block {blk} has the table entry {page}"
        n = min(L - 64 * blk, 64)
        k8.append(state["k_int8"][page, :, 64 * at:64 * at + n])
        ks.append(_f32_of(state["k_scale"][page, :, 4 * at:4 * at + 4]))
        v8.append(util.decode_v_image(state["v_image"][page, :, at:at + 1], 64, True)[:, :n])
    return dict(K8=np.concatenate(k8, axis=1), k_scale=np.concatenate(ks, axis=1), V8=np.concatenate(v8, axis=1), v_scale=_f32_of(state["v_scale"][b]))


def _bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def logical_mismatches(state, page_size, ledger, slots):
    """What differs between the keys a slot's table serves and the ledger's operands: a list of messages, empty when they agree.  ``v_scale`` is
    held to the ledger for slots that hold a row: ``seed`` leaves it as it was, stale until the slot's next append (which is what gives an
    empty slot its first row), and a call reads no ``v_scale`` of a slot without keys to any effect (``o = 0``)."""
    out = []
    for b in slots:
        want = ledger.operands(b)
        if int(state["lens"][b]) != ledger.length(b):
            out.append(f"lens of slot {b}: {int(state['lens'][b])}, the ledger holds {ledger.length(b)} rows")
            continue
        try:
            got = logical(state, page_size, b)
        except AssertionError as e:
            out.append(str(e))
            continue
        for name in ("K8", "k_scale", "V8") + (("v_scale",) if ledger.length(b) else ()):
            diff = _bits_of(got[name]) != _bits_of(want[name])
            if diff.any():
                out.append(f"{name} of slot {b}: {int(diff.sum())} of {diff.size} elements differ, first at {[int(i[0]) for i in diff.nonzero()]}")
    return out


def state_mismatches(got, want, skip_tail_rows_behind=None):
    """Where two states differ, tensor by tensor, naming the pages (pool tensors) or slots (per-slot tensors): a list of messages.
    ``skip_tail_rows_behind``: None, or per-slot row counts -- tail rows at or behind them are not compared."""
    out = []
    for key in KEYS:
        if want[key] is None or got[key] is None:
            if (want[key] is None) != (got[key] is None):
                out.append(f"{key}: one side is None")
            continue
        a, b = _bits_of(got[key]), _bits_of(want[key])
        if a.shape != b.shape:
            out.append(f"{key}: shape {a.shape}, expected {b.shape}")
            continue
        diff = a != b
        if skip_tail_rows_behind is not None and key in ("k_tail", "v_tail"):
            for s, n in enumerate(skip_tail_rows_behind):
                diff[s, :, n:] = False
        if diff.any():
            where = sorted({int(i) for i in diff.nonzero()[0]}) if diff.ndim > 1 else [int(i) for i in diff.nonzero()[0]]
            unit = "pages" if key in ("k_int8", "k_scale", "v_image") else "slots"
            out.append(f"{key}: {int(diff.sum())} elements differ in {unit} {where}, first at {[int(i[0]) for i in diff.nonzero()]}")
    return out


def untouched_pages_mismatches(state, handed_out):
    """Every pool page the allocator never handed out still holds the poison."""
    rest = sorted(set(range(state["k_int8"].shape[0])) - set(handed_out))
    out = []
    for key in ("k_int8", "k_scale", "v_image"):
        bad = [p for p in rest if (np.ascontiguousarray(state[key][p]).view(np.uint8) != POISON).any()]
        if bad:
            out.append(f"{key}: pages {bad} were never handed out and lost their poison")
    return out


# ---------------------------------------------------------------------------------------------------------------- random programs
def _perm(num_pages):
    return [(13 * i + 5) % num_pages for i in range(num_pages)]


class _Pool:
    """The test's allocator: a free list in a fixed order, reference counts on shared pages; a freed page is the next one handed out, with
    its old bytes in it."""

    def __init__(self, num_pages, nslots, max_pages, page_size):
        self.free, self.ref, self.handed, self.dry = _perm(num_pages), {}, set(), False
        self.table = [[None] * max_pages for _ in range(nslots)]
        self.page_size = page_size

    def take(self):
        if not self.free:
            self.dry = True
            return None
        p = self.free.pop(0)
        self.ref[p] = 1
        self.handed.add(p)
        return p

    def release(self, b):
        for e, p in enumerate(self.table[b]):
            if p is not None:
                self.ref[p] -= 1
                if self.ref[p] == 0:
                    del self.ref[p]
                    self.free.insert(0, p)
                self.table[b][e] = None

    def serve(self, b, len0, len1, writes):
        """Pages for rows len0 .. len1 - 1 of slot b; the table entries written go to ``writes``.  Returns the length actually served."""
        for e in range(len0 // self.page_size, (len1 + self.page_size - 1) // self.page_size if len1 > len0 else 0):
            if self.table[b][e] is None:
                p = self.take()
                if p is None:
                    return max(len0, e * self.page_size)
                self.table[b][e] = p
                writes.append((b, e, p))
        return len1


def _targets(page_size):
    return sorted({1, 63, 64, 65, page_size - 1, page_size, page_size + 1, 2 * page_size - 1, 2 * page_size + 1, 200, 330, 449, CAP})


def _count_towards(rng, len0, page_size, most):
    """A row count for a slot that holds len0 rows, biased to land its length on a block, page or capacity edge."""
    ahead = [t - len0 for t in _targets(page_size) if 0 < t - len0 <= most]
    if ahead and rng.random() < 0.65:
        return rng.choice(ahead)
    return rng.randint(1, most)


def random_program(seed):
    """(shape, steps) of program ``seed``: pure Python.  ``shape``: D, code (0 fp16 / 1 bf16), smooth_k, group, page_size, max_pages,
    num_pages, table (the initial block table: -1 and num_pages in turn).  A step is a dict with ``op`` in MUTATING or "attn"; a mutating step
    carries ``table`` -- the entries (slot, entry, page) its caller writes first -- and the lengths every slot holds afterwards (``lens``)."""
    rng = random.Random(52000 + seed)
    page_size = PAGE_SIZES[seed % 3]
    shape = dict(D=(64, 128)[seed & 1], code=(seed >> 1) & 1, smooth_k=bool((seed + (seed >> 2)) & 1), group=(4, 1)[(seed // 3) & 1],
                 page_size=page_size, max_pages=CAP // page_size, num_pages=NSLOTS * CAP // page_size + SPARE_PAGES, seed=seed)
    shape["table"] = [(-1, shape["num_pages"])[(b * shape["max_pages"] + e) & 1] for b in range(NSLOTS) for e in range(shape["max_pages"])]
    pool = _Pool(shape["num_pages"], NSLOTS, shape["max_pages"], page_size)
    lens = [0] * NSLOTS
    steps, n_ops = [], rng.randint(10, 14)
    saturated, pair, attn_no = False, None, 0

    def append_step(packed, want):
        """An append that gives slot b ``want[b]`` rows (before the clamps): dense with T and new_lens, or packed with counts and max_new."""
        nonlocal saturated
        writes = []
        if packed:
            max_new = max(1, max(want))
            if rng.random() < 0.3 and max(want) > 2:
                max_new = max(want) - rng.randint(1, 2)                       # a count above max_new
            eff = [min(w, max_new) for w in want]
            step = dict(op="append_varlen", counts=list(want), max_new=max_new, lead=rng.choice((0, 0, 3)), slack=rng.choice((0, 2)))
        else:
            T = max(1, max(want))
            raw = [w if w < T or rng.random() < 0.7 else T + rng.randint(1, 9) for w in want]      # values above T
            raw = [(-2 if rng.random() < 0.3 else 0) if w == 0 else w for w in raw]
            eff = [max(0, min(r, T)) for r in raw]
            step = dict(op="append", T=T, new_lens=raw if (rng.random() < 0.85 or min(eff) < T) else None, i64=rng.random() < 0.3)
        given = []
        overflow = any(lens[b] + eff[b] > CAP for b in range(NSLOTS))
        for b in range(NSLOTS):
            len1 = min(lens[b] + eff[b], CAP)
            pool.serve(b, lens[b], len1, writes)
            given.append(len1 - lens[b])
            lens[b] = len1
        # (a pool that runs dry leaves table entries outside the pool: the device drops those blocks while lens advance; every live page
        #  stands in some slot's table, so 6 x max_pages pages always suffice -- the program records ``dry`` and tests/test_kvcache_sim_host.py
        #  asserts that no default seed gets there)
        step.update(table=writes, overflow=overflow, sat=None, given=given)
        if not saturated and rng.random() < 0.12:
            takers = [b for b in range(NSLOTS) if eff[b] > 0]
            if takers:
                step["sat"], saturated = rng.choice(takers), True
        return step

    def draw_wants(must=()):
        most = rng.choice((1, 7, 40, 64, 130, 130))
        want = []
        for b in range(NSLOTS):
            if b in must or rng.random() < 0.6:
                want.append(min(_count_towards(rng, lens[b], page_size, most) if lens[b] < CAP else rng.randint(1, most), most))
            else:
                want.append(0)
        if max(want) == 0:
            want[rng.randrange(NSLOTS)] = rng.randint(1, most)
        return want

    def prefill_step(slots):
        writes, rows = [], {}
        for b in slots:
            pool.release(b)
            lens[b] = 0
            rows[b] = rng.choice((1, 63, 64, 65, page_size - 1, page_size + 1, 130, rng.randint(1, 130), 129, 200, 330, 385, 449, 500))
            pool.serve(b, 0, rows[b], writes)
            lens[b] = rows[b]
        return dict(op="prefill", rows=rows, headroom=rng.choice(HEADROOMS), packed=rng.random() < 0.5, table=writes, overflow=False, sat=None,
                    given=[rows.get(b, 0) for b in range(NSLOTS)])

    def fork_step():
        nonlocal pair
        live = [b for b in range(NSLOTS) if lens[b] > 0] or [0]
        src0 = rng.choice(live)
        others = sorted((b for b in range(NSLOTS) if b != src0), key=lambda b: (lens[b], rng.random()))
        n = 2 if rng.random() < 0.3 else 1
        dst = others[:n]
        src = [src0] + ([rng.choice([src0] + [b for b in live if b not in dst])] if n == 2 else [])
        prefix = None
        if rng.random() < 0.6:
            prefix = []
            for s in src:
                L = lens[s]
                prefix.append(rng.choice((L, L // 64 * 64, max(L - 3, 0), 64, 65, L + 5, page_size, -1)))
        writes, pages = [], []
        for i, (s, d) in enumerate(zip(src, dst)):
            pool.release(d)
            P = prefix_len(lens[s], None if prefix is None else prefix[i])
            whole = P // page_size
            for e in range(whole):
                pool.table[d][e] = pool.table[s][e]
                pool.ref[pool.table[s][e]] += 1
            if whole < shape["max_pages"]:
                p = pool.take()
                pool.table[d][whole] = p
            else:
                p = next(f for f in pool.free if f not in pages)       # (the table has no entry for it: the page stays free)
            pages.append(p)
            lens[d] = P
        pair = (src[0], dst[0])
        return dict(op="fork", src=src, dst=dst, pages=pages, prefix=prefix, tensors=rng.choice((None, "i32", "i64")), table=writes, overflow=False, sat=None)

    def reseed_step():
        slots = rng.sample(range(NSLOTS), rng.choice((1, 1, 2)))
        busiest = max(range(NSLOTS), key=lambda b: lens[b])
        if busiest not in slots and rng.random() < 0.5:
            slots[0] = busiest
        for b in slots:
            pool.release(b)
            lens[b] = 0
        return dict(op="reseed", slots=sorted(slots), factor=rng.choice((0.5, 1.0, 2.0)), table=[], overflow=False, sat=None)

    def attn_step():
        nonlocal attn_no
        route = ROUTES[(3 * seed + 7 * attn_no + rng.randrange(3)) % len(ROUTES)]
        attn_no += 1
        if shape["group"] == 1 and route == "dense_pack":
            route = "dense_br"
        elif shape["group"] > 1 and rng.random() < 0.15:
            route = "dense_pack"
        step = dict(op="attn", route=route, window=None, q_start=None, splits=None, pack=False)
        if route.startswith("varlen"):
            counts = [rng.choice(VARLEN_LQS) for _ in range(NSLOTS)]
            if max(counts) == 0:
                counts[rng.randrange(NSLOTS)] = rng.choice(VARLEN_LQS[1:])
            step.update(counts=counts, lead=rng.choice((0, 0, 2)), slack=rng.choice((0, 3)))
            if route == "varlen_window":
                step["window"] = rng.choice((0, 1, 37, 64, 100, 300))
            if route == "varlen_qstart":
                step["q_start"] = [rng.choice((0, lens[b] - c, lens[b] - c - 5, 3, -7, rng.randint(-20, CAP))) for b, c in enumerate(counts)]
            return step
        if route == "split":
            step.update(Lq=rng.choice(DENSE_LQS[:3]), splits=rng.choice(SPLITS), mask=rng.choice(("nc", "tl", "br", "qstart")))
            step["pack"] = shape["group"] > 1 and step["Lq"] <= 32 and rng.random() < 0.4
        elif route == "dense_pack":
            step.update(Lq=rng.choice(DENSE_LQS[:2]), mask=rng.choice(("nc", "br", "qstart", "window")), pack=True)
        else:
            step.update(Lq=rng.choice(DENSE_LQS), mask=dict(dense_nc="nc", dense_tl="tl", dense_br="br", dense_qstart="qstart", dense_window="window")[route])
        if step["mask"] == "qstart":
            step["q_start"] = [rng.choice((lens[b] - step["Lq"], lens[b] - step["Lq"] + 2, 0, 5, -3, rng.randint(-step["Lq"], CAP))) for b in range(NSLOTS)]
        if step["mask"] == "window":
            step["window"] = rng.choice((0, 1, 37, 64, 100, 300))
            step["align"] = rng.choice(("tl", "br", "qstart"))
            if step["align"] == "qstart":
                step["q_start"] = [rng.choice((lens[b] - step["Lq"], 0, 7, rng.randint(-step["Lq"], CAP))) for b in range(NSLOTS)]
        return step

    # the first step fills some slots from their first rows; a fork, appends to both sides of it and an attention step follow in most programs;
    # the rest is drawn; the last step is an attention step
    script = ["append" if rng.random() < 0.5 else "append_varlen", "fork", "both", "attn"] if rng.random() < 0.85 else []
    extras = [rng.choice(("append", "append_varlen", "append", "append_varlen", "fork", "reseed", "reseed", "prefill", "attn", "attn", "attn", "overflow", "overflow"))
              for _ in range(n_ops - 2 - len(script))]
    cut = rng.randint(0, min(2, len(extras)))
    plan = ["prefill"] + extras[:cut] + script + extras[cut:] + ["attn"]
    assert len(plan) == n_ops
    for kind in plan:
        if kind == "prefill":
            fresh = [b for b in range(NSLOTS) if lens[b] == 0] or list(range(NSLOTS))
            steps.append(prefill_step(sorted(rng.sample(fresh, min(len(fresh), rng.randint(2, 4))))))
        elif kind in ("append", "append_varlen"):
            steps.append(append_step(kind == "append_varlen", draw_wants(pair if pair and rng.random() < 0.7 else ())))
        elif kind == "both":
            steps.append(append_step(rng.random() < 0.5, draw_wants(pair or ())))
        elif kind == "overflow":
            b = max(range(NSLOTS), key=lambda s: lens[s])
            want = draw_wants()
            room = CAP - lens[b]
            want[b] = min(130, room + rng.randint(1, 20)) if room < 130 else 130
            for s in range(NSLOTS):                 # (long rows for the slots near the capacity, so that the clamp runs)
                if CAP - lens[s] < want[b]:
                    want[s] = max(want[s], min(want[b], CAP - lens[s] + 3))
            steps.append(append_step(rng.random() < 0.5, want))
        elif kind == "fork":
            steps.append(fork_step())
        elif kind == "reseed":
            steps.append(reseed_step())
        else:
            steps.append(attn_step())
        steps[-1]["lens"] = list(lens)
        steps[-1]["handed"] = sorted(pool.handed)
    shape["dry"] = pool.dry
    return shape, steps


def contiguous_variant(shape, steps):
    """The program with the fork, packed and paging operations filtered out, for a contiguous ``QuantizedKVCache``: a prefill appends densely,
    packed appends become dense ones of the same counts, forks and the packed attention steps are dropped; one page of CAP keys per slot."""
    shape = dict(shape, page_size=CAP, max_pages=1, num_pages=NSLOTS, table=list(range(NSLOTS)), contiguous=True)
    lens, out = [0] * NSLOTS, []
    for step in steps:
        step = dict(step, table=[])
        if step["op"] == "fork" or (step["op"] == "attn" and step["route"].startswith("varlen")):
            continue
        if step["op"] == "append_varlen":
            eff = [min(c, step["max_new"]) for c in step["counts"]]
            step = dict(step, op="append", T=max(1, max(eff)), new_lens=eff, i64=False)
        if step["op"] == "append":
            T = step["T"]
            raw = step["new_lens"] if step["new_lens"] is not None else [T] * NSLOTS
            lens = [min(n + max(0, min(r, T)), CAP) for n, r in zip(lens, raw)]
        elif step["op"] == "prefill":
            step = dict(step, packed=False)
            for b, n in step["rows"].items():
                lens[b] = n
        elif step["op"] == "reseed":
            for b in step["slots"]:
                lens[b] = 0
        elif step["op"] == "attn" and step.get("q_start") is not None:
            step = dict(step, q_start=list(step["q_start"]))
        out.append(dict(step, lens=list(lens), handed=list(range(NSLOTS))))
    return shape, out


# ---------------------------------------------------------------------------------------------------------------- a program's concrete arrays
class Run:
    """Program ``(shape, steps)`` made concrete, with the ledger and the simulator in step.  ``action(i)`` returns the arrays of step i (rows,
    statistics, index lists: what a caller hands to the cache under test); ``advance(i, act)`` applies a mutating step to both layers."""

    def __init__(self, oracle, shape, steps, mutant=None):
        self.oracle, self.shape, self.steps = oracle, shape, steps
        self.D, self.code, self.page_size = shape["D"], shape["code"], shape["page_size"]
        rng = np.random.default_rng([91, shape["seed"]])
        self.bias = (1.5 * rng.standard_normal((NSLOTS, HKV, 1, self.D))).astype(np.float32)        # K's per-channel offset, one per slot
        self.chan = (0.25 + rng.random((NSLOTS, HKV, 1, self.D))).astype(np.float32)                # V's per-channel spread
        self.ledger = Ledger(oracle, NSLOTS, HKV, self.D, self.code, shape["max_pages"] * self.page_size)
        self.sim = Simulator(oracle, self.page_size, self.code, mutant)
        self.state = poisoned_state(shape["num_pages"], self.page_size, NSLOTS, shape["max_pages"], HKV, self.D, shape["smooth_k"], shape["table"])
        # the whole cache's first statistics: every slot its own, none taken from content
        self.km0 = to_bits(self.bias[:, :, 0], self.code) if shape["smooth_k"] else None
        self.va0 = (3.0 * self.chan[:, :, 0]).astype(np.float32)
        self.sim.seed(self.state, range(NSLOTS), self.km0, self.va0)
        self.ledger.seed(range(NSLOTS), self.km0, self.va0)

    def _rows(self, i, n, sat=None):
        """Fresh rows for every slot at step i: k, v bit patterns ``[NSLOTS, HKV, n, D]``; ``sat``: that slot's V at 8 x its frozen abs-max."""
        rng = np.random.default_rng([17, self.shape["seed"], i])
        k = rng.standard_normal((NSLOTS, HKV, n, self.D)).astype(np.float32) + self.bias
        v = rng.standard_normal((NSLOTS, HKV, n, self.D)).astype(np.float32) * self.chan
        if sat is not None:
            v[sat] = np.where(v[sat] < 0, -8.0, 8.0).astype(np.float32) * self.ledger.v_amax[sat][:, None, :]
        return to_bits(k, self.code), to_bits(v, self.code)

    def _pack(self, i, k, v, counts, lead, slack):
        cu = [lead]
        for c in counts:
            cu.append(cu[-1] + c)
        total = max(cu[-1] + slack, 1)
        kp, vp = self._rows(1000 + i, total)                 # (rows no slot owns: random data too)
        kp, vp = np.swapaxes(kp[0], 0, 1).copy(), np.swapaxes(vp[0], 0, 1).copy()
        for b, c in enumerate(counts):
            kp[cu[b]:cu[b + 1]] = np.swapaxes(k[b, :, :c], 0, 1)
            vp[cu[b]:cu[b + 1]] = np.swapaxes(v[b, :, :c], 0, 1)
        return kp, vp, cu

    def action(self, i):
        step = self.steps[i]
        op = step["op"]
        act = dict(op=op, table=step.get("table", []))
        if op == "append":
            act["k"], act["v"] = self._rows(i, step["T"], step["sat"])
            act.update(new_lens=step["new_lens"], i64=step["i64"])
        elif op == "append_varlen":
            n = max(1, max(step["counts"]))
            k, v = self._rows(i, n, step["sat"])
            act["k"], act["v"], act["cu"] = self._pack(i, k, v, step["counts"], step["lead"], step["slack"])
            act["max_new"] = step["max_new"]
        elif op == "prefill":
            slots = sorted(step["rows"])
            n = max(step["rows"].values())
            k, v = self._rows(i, n)
            km, va = [], []
            for b in slots:
                r = step["rows"][b]
                km.append(to_bits(util.f32(k[b, :, :r], self.code).astype(np.float64).mean(axis=1).astype(np.float32), self.code))
                va.append((np.abs(util.f32(v[b, :, :r], self.code)).max(axis=1) * np.float32(step["headroom"])).astype(np.float32))
            counts = [step["rows"].get(b, 0) for b in range(NSLOTS)]
            act.update(slots=slots, k_mean=np.stack(km) if self.shape["smooth_k"] else None, v_amax=np.stack(va), counts=counts, packed=step["packed"])
            if step["packed"]:
                act["k"], act["v"], act["cu"] = self._pack(i, k, v, counts, 0, 0)
                act["max_new"] = n
            else:
                act["k"], act["v"] = k, v
        elif op == "reseed":
            slots = step["slots"]
            rng = np.random.default_rng([23, self.shape["seed"], i])
            km = to_bits(self.bias[slots, :, 0] + 0.1 * rng.standard_normal((len(slots), HKV, self.D)).astype(np.float32), self.code)
            act.update(slots=slots, k_mean=km if self.shape["smooth_k"] else None, v_amax=(3.0 * step["factor"] * self.chan[slots, :, 0]).astype(np.float32))
        elif op == "fork":
            act.update(src=step["src"], dst=step["dst"], pages=step["pages"], prefix=step["prefix"], tensors=step["tensors"])
        else:
            rng = np.random.default_rng([29, self.shape["seed"], i])
            Hq = HKV * self.shape["group"]
            act.update(step)
            if step["route"].startswith("varlen"):
                cu = [step["lead"]]
                for c in step["counts"]:
                    cu.append(cu[-1] + c)
                act["cu"], act["total"] = cu, cu[-1] + step["slack"]
                act["q"] = to_bits(rng.standard_normal((act["total"], Hq, self.D)).astype(np.float32), self.code)
            else:
                act["q"] = to_bits(rng.standard_normal((NSLOTS, Hq, step["Lq"], self.D)).astype(np.float32), self.code)
        return act

    def advance(self, i, act):
        """Apply mutating step i to the simulator's state and to the ledger (the table entries its caller writes first)."""
        op, sim, led, st = act["op"], self.sim, self.ledger, self.state
        for b, e, p in act["table"]:
            st["block_table"][b, e] = p
        if op in ("prefill", "reseed"):
            sim.seed(st, act["slots"], act["k_mean"], act["v_amax"])
            led.seed(act["slots"], act["k_mean"], act["v_amax"])
        if op == "append" or (op == "prefill" and not act["packed"]):
            new_lens = act["new_lens"] if op == "append" else act["counts"]
            T = act["k"].shape[2]
            sim.append(st, act["k"], act["v"], new_lens)
            for b in range(NSLOTS):
                n = T if new_lens is None else max(0, min(int(new_lens[b]), T))
                led.append(b, act["k"][b, :, :n], act["v"][b, :, :n])
        elif op == "append_varlen" or op == "prefill":
            sim.append_varlen(st, act["k"], act["v"], act["cu"], act["max_new"])
            for b in range(NSLOTS):
                n = max(0, min(act["cu"][b + 1] - act["cu"][b], act["max_new"]))
                led.append(b, np.swapaxes(act["k"][act["cu"][b]:act["cu"][b] + n], 0, 1), np.swapaxes(act["v"][act["cu"][b]:act["cu"][b] + n], 0, 1))
        elif op == "fork":
            sim.fork(st, act["src"], act["dst"], act["pages"], act["prefix"])
            for j, (s, d) in enumerate(zip(act["src"], act["dst"])):
                led.fork(s, d, None if act["prefix"] is None else act["prefix"][j])

    def check(self, i):
        """The simulator's own proof after step i: the keys every slot's table serves are the ledger's, the planned lengths hold, and the pages
        never handed out keep their poison.  A list of messages."""
        step = self.steps[i]
        out = [f"step {i} ({step['op']}): {m}" for m in logical_mismatches(self.state, self.page_size, self.ledger, range(NSLOTS))]
        if [self.ledger.length(b) for b in range(NSLOTS)] != step["lens"]:
            out.append(f"step {i} ({step['op']}): the ledger holds {[self.ledger.length(b) for b in range(NSLOTS)]} rows, the program planned {step['lens']}")
        return out + [f"step {i} ({step['op']}): {m}" for m in untouched_pages_mismatches(self.state, step["handed"])]


def attn_geometry(step, b, L):
    """(Lq, window_size pair, is_causal, q_start) of slot b in attention step ``step`` -- the public meaning of the keywords it is called with;
    ``L``: the keys the slot holds.  Bottom-right: ``q_start = L - Lq``."""
    if step["route"].startswith("varlen"):
        Lq = step["counts"][b]
        start = L - Lq if step["q_start"] is None else step["q_start"][b]
        return Lq, ((step["window"], 0) if step["window"] is not None else (-1, -1)), True, start
    Lq, mask = step["Lq"], step["mask"]
    if mask == "window":
        mask = step["align"]
    start = dict(nc=0, tl=0, br=L - Lq, qstart=None)[mask]
    if start is None:
        start = step["q_start"][b]
    window = (step["window"], 0) if step["window"] is not None else (-1, -1)
    return Lq, window, step["mask"] != "nc", start
