"""A fenced, poisoned allocator for tests: every device buffer the package allocates sits between two guard regions, and ``check()`` proves that
nothing wrote into them.

The kernels form their addresses by hand (prefetch two tiles ahead, clamped row offsets in ragged tiles, biased base pointers, per-lane source
offsets, packed sequences side by side).  A store one row too far, or a load past the end whose value is used, lands in whatever the caching
allocator put next to the buffer -- invisible on random data.  Under the fence

  * every allocation made through ``torch.empty`` / ``torch.zeros`` / ``torch.empty_like`` (the functions ``sageattention_amd`` reaches device
    memory with, looked up as ``torch.<name>``) becomes one byte arena ``guard | body | guard``; the body is returned as the tensor asked for;
  * the guards -- and the body of an ``empty`` -- hold the fill byte: ``0xFF`` (NaN as fp16 / bf16 / fp32 / e4m3, -1 as int8 / int32) or ``0x5A``
    (finite; the pattern of the allocator soak test).  A stray store changes a guard byte (``check()`` fails); a stray load that is used reads
    NaN under one fill and a finite value under the other, so the result differs between the fills, or from the unfenced run;
  * ``GUARD`` is 64 KiB: more than two pipeline stages of the largest instantiation -- a K tile of 8 KiB plus an fp16 V image tile of 16 KiB,
    two tiles ahead = 48 KiB -- so any stray access of the prefetch distance the loops use lands inside it; a multiple of 128, so the body keeps
    the 128-byte alignment that the ticket workspace needs.

CPU allocations, zero-sized ones, anything under graph capture and any call with arguments the fence does not model (``out=``, pinned memory,
a non-strided layout) pass through untouched.  What torch allocates itself (``F.pad``, ``.contiguous()``, ``.to()``, arithmetic) is not fenced.

What it cannot see: a load past the end whose value is never used (masked key rows, whose score is replaced in front of the row maximum;
prefetched tiles that are never consumed).  Only used loads and all stores are covered.

Not a conftest: test modules import it explicitly.
"""
import os
import sys

import torch

GUARD = 64 * 1024
ALIGN = 128
FILLS = (0xFF, 0x5A)

_PKG = "sageattention_amd"
_HERE = os.path.abspath(__file__)


class FenceViolation(AssertionError):
    pass


class _Arena:
    """One allocation: ``arena`` (uint8) = pad | guard | body | guard; ``lo`` is the body's byte offset inside it."""
    __slots__ = ("arena", "lo", "nbytes", "shape", "dtype", "site", "func", "in_pkg", "kind", "gap")

    def describe(self):
        return f"{self.kind} {tuple(self.shape)} {str(self.dtype).replace('torch.', '')} allocated at {self.site}"

    def guards(self):
        return (("below", self.arena[self.lo - GUARD:self.lo]), ("above", self.arena[self.lo + self.nbytes:self.lo + self.nbytes + GUARD]))


def _is_cuda(dev: torch.device) -> bool:
    return dev.type == "cuda"


def _site():
    """(file:line, function, inside the package?) of the innermost frame inside ``sageattention_amd``; else of the first frame outside this module."""
    f = sys._getframe(1)
    first_outside = None
    while f is not None:
        fn = os.path.abspath(f.f_code.co_filename)
        if fn != _HERE:
            parts = fn.split(os.sep)
            if _PKG in parts[:-1]:
                return f"{_PKG}/{'/'.join(parts[parts.index(_PKG) + 1:])}:{f.f_lineno}", f.f_code.co_name, True
            if first_outside is None:
                first_outside = (f"{os.path.basename(fn)}:{f.f_lineno}", f.f_code.co_name)
        f = f.f_back
    return (*(first_outside or ("<unknown>", "<unknown>")), False)


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


class Fence:
    """``with Fence(fill) as f: out = call(f.input(q), ...); f.check()`` -- see the module docstring.  ``device_ok``: which devices are fenced
    (the default: CUDA; the CPU self-tests of this helper pass ``lambda d: True``)."""

    def __init__(self, fill: int, device_ok=_is_cuda):
        assert 0 <= fill <= 0xFF
        self.fill = int(fill)
        self.device_ok = device_ok
        self.arenas = []
        self._saved = None

    # ------------------------------------------------------------------------------------------------ context
    def __enter__(self):
        assert self._saved is None, "a Fence is entered once"
        self._drop_cache()
        self._saved = (torch.empty, torch.zeros, torch.empty_like)
        torch.empty, torch.zeros, torch.empty_like = self._empty, self._zeros, self._empty_like
        return self

    def __exit__(self, *exc):
        torch.empty, torch.zeros, torch.empty_like = self._saved
        self._drop_cache()          # no fenced ticket / pre-pass block outlives the test
        self.arenas = []
        return False

    @staticmethod
    def _drop_cache():
        from sageattention_amd import _stream_cache
        with _stream_cache._LOCK:
            _stream_cache._CACHE.clear()

    # ------------------------------------------------------------------------------------------------ allocation
    def _fenceable(self, shape, kw):
        """The device to fence this allocation on, or None (pass through)."""
        if any(kw.get(n) is not None for n in ("out", "names")) or kw.get("pin_memory") or kw.get("requires_grad"):
            return None
        if kw.get("layout", torch.strided) is not torch.strided:
            return None
        if kw.get("memory_format", torch.contiguous_format) not in (torch.contiguous_format, torch.preserve_format):
            return None
        dev = kw.get("device")
        dev = torch.device(dev) if dev is not None else torch.get_default_device()
        if dev.type == "meta" or not self.device_ok(dev):
            return None
        n = 1
        for s in shape:
            n *= s
        if n == 0:
            return None
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return None
        return dev

    def _arena(self, shape, dtype, dev, kind, zero=False):
        """Allocate guard | body | guard on ``dev`` and record it; returns (record, flat body of ``dtype``)."""
        e, z, _ = self._saved
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * dtype.itemsize
        raw = e(ALIGN + 2 * GUARD + nbytes, dtype=torch.uint8, device=dev)
        raw.fill_(self.fill)
        r = _Arena()
        r.arena, r.nbytes, r.shape, r.dtype, r.kind, r.gap = raw, nbytes, tuple(shape), dtype, kind, None
        r.lo = (-raw.data_ptr()) % ALIGN + GUARD
        r.site, r.func, r.in_pkg = _site()
        body = raw[r.lo:r.lo + nbytes]
        if zero:
            body.zero_()
        self.arenas.append(r)
        return r, body.view(dtype)

    def _empty(self, *size, **kw):
        shape = _shape_of(size) if size else _shape_of((kw.pop("size"),))
        dev = self._fenceable(shape, kw)
        if dev is None:
            return self._saved[0](shape, **kw)
        return self._arena(shape, kw.get("dtype"), dev, "empty")[1].view(shape)

    def _zeros(self, *size, **kw):
        shape = _shape_of(size) if size else _shape_of((kw.pop("size"),))
        dev = self._fenceable(shape, kw)
        if dev is None:
            return self._saved[1](shape, **kw)
        return self._arena(shape, kw.get("dtype"), dev, "zeros", zero=True)[1].view(shape)

    def _empty_like(self, t, **kw):
        kw2 = dict(kw)
        kw2.setdefault("device", t.device)
        dev = self._fenceable(tuple(t.shape), kw2) if t.layout is torch.strided else None
        if dev is None:
            return self._saved[2](t, **kw)
        dtype = kw.get("dtype") or t.dtype
        # the strides torch.empty_like would give (preserve_format: those of a dense, non-overlapping input; else contiguous)
        strides = self._saved[2](t, device="meta", memory_format=kw.get("memory_format", torch.preserve_format)).stride()
        return self._arena(tuple(t.shape), dtype, dev, "empty_like")[1].as_strided(tuple(t.shape), strides)

    # ------------------------------------------------------------------------------------------------ caller tensors
    def output(self, shape, dtype, gap_rows: int = 0, tensor_layout: str = "HND", device=None):
        """A caller-provided buffer inside an arena, every byte the fill.  ``gap_rows`` > 0 (dense 4-D): the view ``[:, :, :L]`` (HND) or
        ``[:, :L]`` (NHD) of a buffer with ``gap_rows`` more rows along the sequence.  HND: every head -- not only the last one -- ends in
        guard rows.  NHD: heads are interleaved token by token, so the guard rows (of all heads) sit behind every batch's ``[L, H, D]`` block.
        ``check()`` covers them.  Strides stay multiples of 8 elements for every head dim that is one."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        shape = tuple(int(s) for s in shape)
        if not gap_rows:
            return self._arena(shape, dtype, dev, "caller tensor")[1].view(shape)
        assert len(shape) == 4 and tensor_layout in ("HND", "NHD"), "gap rows: a dense 4-D tensor"
        seq = 2 if tensor_layout == "HND" else 1
        L = shape[seq]
        full = list(shape)
        full[seq] = L + int(gap_rows)
        r, body = self._arena(tuple(full), dtype, dev, "caller tensor with gap rows")
        buf = body.view(full)
        r.shape = shape
        r.gap = buf.narrow(seq, L, int(gap_rows))
        return buf.narrow(seq, 0, L)

    def input(self, t: torch.Tensor, gap_rows: int = 0, tensor_layout: str = "HND", device=None):
        """``t`` (from any device) copied into an arena on ``device`` (the default: the current CUDA device): see :meth:`output`.  A
        non-contiguous dense ``t`` keeps its strides when ``gap_rows`` is 0."""
        if gap_rows or t.is_contiguous():
            dst = self.output(t.shape, t.dtype, gap_rows, tensor_layout, device)
        else:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            strides = self._saved[2](t, device="meta").stride()
            dst = self._arena(tuple(t.shape), t.dtype, dev, "caller tensor")[1].as_strided(tuple(t.shape), strides)
        dst.copy_(t)
        return dst

    # ------------------------------------------------------------------------------------------------ checks
    def owns(self, t: torch.Tensor) -> bool:
        """Whether ``t``'s storage is one of the arenas."""
        p = t.untyped_storage().data_ptr()
        return any(r.arena.untyped_storage().data_ptr() == p for r in self.arenas)

    def package_sites(self):
        """The allocation sites inside ``sageattention_amd`` recorded so far."""
        return [r.site for r in self.arenas if r.in_pkg]

    def package_allocations(self):
        """(function, shape, dtype) of every allocation made from inside ``sageattention_amd`` so far: which route ran shows in what it allocated."""
        return [(r.func, r.shape, r.dtype) for r in self.arenas if r.in_pkg]

    def check(self):
        """Synchronise, then assert that every guard byte (and every gap row) of every recorded arena still holds the fill.  The failure
        names the allocation site, shape and dtype, the side, and the first and last changed byte relative to the buffer's edge: below,
        -1 is the byte in front of the body's first; above, +0 is the first byte behind its last."""
        if torch.cuda.is_available() and any(r.arena.is_cuda for r in self.arenas):
            torch.cuda.synchronize()
        # one host synchronisation for the common case: the number of changed bytes over all guards and gaps, summed on the device
        counts = [(g != self.fill).sum() for r in self.arenas for _, g in r.guards()]
        counts += [(r.gap.contiguous().view(torch.uint8) != self.fill).sum() for r in self.arenas if r.gap is not None]
        if not counts or int(torch.stack([c.to(counts[0].device) for c in counts]).sum()) == 0:
            return
        problems = []
        for r in self.arenas:
            for side, g in r.guards():
                bad = g != self.fill
                if bool(bad.any()):
                    idx = bad.nonzero().flatten()
                    first, last = int(idx[0]), int(idx[-1])
                    if side == "below":
                        first, last = first - GUARD, last - GUARD
                    problems.append(f"{r.describe()}: {int(idx.numel())} guard byte(s) {side} the buffer changed, "
                                    f"first at {first:+d}, last at {last:+d} (fill 0x{self.fill:02X})")
            if r.gap is not None:
                gb = r.gap.contiguous().view(torch.uint8)
                bad = gb != self.fill
                if bool(bad.any()):
                    idx = bad.nonzero()
                    problems.append(f"{r.describe()}: {int(idx.shape[0])} byte(s) of the gap rows changed, first at index {tuple(int(i) for i in idx[0])}, "
                                    f"last at {tuple(int(i) for i in idx[-1])} of the gap {tuple(gb.shape)} (fill 0x{self.fill:02X})")
        if problems:
            raise FenceViolation("out-of-bounds write: " + "; ".join(problems))


def fenced_input(fence: Fence, t: torch.Tensor, gap_rows: int = 0, tensor_layout: str = "HND", device=None):
    """``fence.input``: a copy of a caller tensor inside an arena of ``fence`` (with ``gap_rows`` guard rows behind every head, HND, or every batch, NHD)."""
    return fence.input(t, gap_rows, tensor_layout, device)
