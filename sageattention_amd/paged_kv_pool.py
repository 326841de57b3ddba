"""A device-side page pool for the paged quantised KV cache: a free stack, reference counts and the block table kept by the lengths (gfx950
extension).

:class:`~sageattention_amd.paged_kv_cache.PagedQuantizedKVCache` reads a ``block_table`` the caller writes and :meth:`fork` takes the child's
page from the caller: which pages are free, and when a shared page may be reused, is host bookkeeping between two launches -- so a captured
step cannot grow a sequence across a page boundary.  :class:`PagePool` keeps that bookkeeping in one int32 workspace on the device
(``include/sage_kvpool_gfx950.h``): one small launch in front of an append hands every slot the pages its new rows need, one in front of a fork
counts the shared pages and hands the child its own, and a release returns the pages whose last reference went.  Nothing is read on the host;
a captured ``pool.append`` + attention step replays through page boundaries.

The cache class itself is unchanged and the pool is a default of nothing: a cache a :class:`PagePool` manages must not have its table written
by anyone else.

Import from here (``from sageattention_amd.paged_kv_pool import PagePool``); the name is not part of the package's ``__all__``.  Not under
torch.compile.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _cabi, _cabi_kvpool
from .kv_cache import _dims, _is_int
from .paged_kv_cache import PagedQuantizedKVCache
from .quant import _p, _stream

__all__ = ["PagePool"]

MAX_SLOTS = 1024      # kVarlenPlanMaxSeq: the slots (forks) one launch of one workgroup takes
HDR_WORDS = 16


class PagePool:
    """The pages of ``cache`` (a :class:`PagedQuantizedKVCache` whose ``block_table`` is still its fresh -1 fill, at most 1024 slots).

    ``ws`` int32 ``[16 + 2 * num_pages + B]`` on the cache's device is the whole state: ``hdr`` (``n_free``, the slots the last call refused,
    the pages it was short of, refusals since :meth:`init`), ``free_stack`` (the top, ``free_stack[n_free - 1]``, is handed out next; page 0
    first), ``refcount`` and ``n_owned`` -- views of it under those names.  Every method but :meth:`status` is one small launch (plus the
    cache's own) on the current stream, reads nothing on the host and captures into a HIP graph.  (``_init=False`` leaves the workspace as
    allocated: the tests' workspace that ``init`` never wrote.)"""

    def __init__(self, cache, _init: bool = True):
        if not isinstance(cache, PagedQuantizedKVCache):
            raise ValueError(f"PagePool takes a PagedQuantizedKVCache (got {type(cache).__name__})")
        if cache.B > MAX_SLOTS:
            raise ValueError(f"PagePool serves at most {MAX_SLOTS} sequence slots (got B = {cache.B})")
        self.cache = cache
        N, B = cache.num_pages, cache.B
        self.ws = torch.empty((HDR_WORDS + 2 * N + B,), dtype=torch.int32, device=cache.device)
        self.hdr, self.free_stack = self.ws[:HDR_WORDS], self.ws[HDR_WORDS:HDR_WORDS + N]
        self.refcount, self.n_owned = self.ws[HDR_WORDS + N:HDR_WORDS + 2 * N], self.ws[HDR_WORDS + 2 * N:]
        if _init:
            self.init()

    def _geometry(self):
        c = self.cache
        return (_p(self.ws), self.ws.numel() * 4, _p(c.block_table), c.block_table.stride(0), c.num_pages, c.page_size, c.max_pages_per_seq, c.B)

    @torch.compiler.disable
    def init(self) -> None:
        """Every page free, page 0 on top; no slot owns anything.  The table is not touched: it must hold its -1 fill."""
        rc = _cabi_kvpool.load().sage_kvpool_init(_p(self.ws), self.ws.numel() * 4, self.cache.num_pages, self.cache.B, _stream(self.ws))
        _cabi.check(rc, "sage_kvpool_init")

    def _int_array(self, name, t, n, what) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name} must be an int32 or int64 tensor (got {getattr(t, 'dtype', type(t).__name__)})")
        if t.dim() != 1 or t.shape[0] != n:
            raise ValueError(f"{name} must have shape {what} = [{n}] (got {tuple(t.shape)})")
        if t.device != self.cache.device:
            raise ValueError(f"{name} must be on the cache's device {self.cache.device} (got {t.device})")
        if t.dtype == torch.int64:
            t = t.clamp(-2 ** 31, 2 ** 31 - 1)
        return t.to(torch.int32).contiguous()

    @staticmethod
    def _host_int(name, x) -> int:
        if not _is_int(x) or x < 1:
            raise ValueError(f"{name} must be a positive int on the host (got {x!r})")
        return x

    @torch.compiler.disable
    def reserve(self, new_lens: Optional[torch.Tensor] = None, T: Optional[int] = None, cu_seqlens: Optional[torch.Tensor] = None,
                max_new: Optional[int] = None, total: Optional[int] = None) -> torch.Tensor:
        """Pages for the rows an append is about to bring: ``reserve(new_lens=, T=)`` for :meth:`PagedQuantizedKVCache.append` (slot b brings
        ``clamp(new_lens[b], 0, T)`` rows) or ``reserve(cu_seqlens=, max_new=, total=)`` for ``append_varlen`` (``total``: the rows of the
        packed tensor; the append's own clamp of the prefix words).  Slot b needs ``ceil(min(lens[b] + n_b, capacity) / page_size)`` entries
        less those it owns; it is granted iff it needs none or the needs of slots ``0 .. b`` together fit into the free pages -- refused slots'
        needs count, so the granted slots with a need are a prefix of those with one.  Returns ``granted`` int32 ``[B]``: ``n_b`` for a granted
        slot, 0 for a refused one, whose table row is untouched."""
        c = self.cache
        if (new_lens is None) == (cu_seqlens is None):
            raise ValueError("reserve takes exactly one of new_lens (with T) and cu_seqlens (with max_new and total)")
        if new_lens is not None:
            T = self._host_int("T", T)
            new_lens = self._int_array("new_lens", new_lens, c.B, "[B]")
            max_new = total = 1
        else:
            max_new, total = self._host_int("max_new", max_new), self._host_int("total", total)
            cu_seqlens = self._int_array("cu_seqlens", cu_seqlens, c.B + 1, "[B + 1]")
            T = 1
        granted = torch.empty((c.B,), dtype=torch.int32, device=c.device)
        rc = _cabi_kvpool.load().sage_kvpool_reserve(*self._geometry(), _p(c.lens), _p(new_lens), T, _p(cu_seqlens), total, max_new, _p(granted), _stream(self.ws))
        _cabi.check(rc, "sage_kvpool_reserve")
        return granted

    @torch.compiler.disable
    def append(self, k_new: torch.Tensor, v_new: torch.Tensor, new_lens: Optional[torch.Tensor] = None, tensor_layout: str = "HND") -> torch.Tensor:
        """:meth:`reserve`, then ``cache.append(k_new, v_new, new_lens=granted)``: a refused slot appends nothing -- its ``lens``, table row and
        pages are untouched, ``hdr`` counts it and the caller offers its rows again.  Returns ``granted``."""
        c = self.cache
        if not c._seeded:
            raise ValueError("the cache has no statistics yet: seed(k_mean, v_amax) or from_prefill(...) before the first append")
        c._new_rows(k_new, v_new, tensor_layout)
        T = _dims(k_new, tensor_layout)[2]
        if new_lens is None:
            new_lens = torch.full((c.B,), T, dtype=torch.int32, device=c.device)
        granted = self.reserve(new_lens=new_lens, T=T)
        c.append(k_new, v_new, new_lens=granted, tensor_layout=tensor_layout)
        return granted

    @torch.compiler.disable
    def append_varlen(self, k_new: torch.Tensor, v_new: torch.Tensor, cu_seqlens: torch.Tensor, max_new: int) -> torch.Tensor:
        """:meth:`reserve` of the packed form, then :func:`~sageattention_amd.paged_kv_varlen.append_varlen`, which takes its row counts from
        ``cu_seqlens`` and not from ``granted``.  **A refused slot's rows are therefore dropped by the append's own rule for a page id of -1
        while its ``lens`` advance**: the slot no longer holds what its length says.  ``hdr[1]`` and the returned ``granted`` say so, and the
        slot is to be released (and its sequence offered again).  Returns ``granted``."""
        from .paged_kv_varlen import _packed, append_varlen
        _packed("k_new", k_new, self.cache.Hkv, self.cache)
        granted = self.reserve(cu_seqlens=cu_seqlens, max_new=max_new, total=int(k_new.shape[0]))
        append_varlen(self.cache, k_new, v_new, cu_seqlens, max_new)
        return granted

    def _slots(self, name, x, what) -> tuple:
        """(int32 tensor [n] on the device, the ints it was given as or None): a sequence of ints is checked here, a tensor is never read."""
        c = self.cache
        t, values = c._fork_index(name, x, c.B, what)
        n = int(t.shape[0])
        if n < 1 or n > MAX_SLOTS:
            raise ValueError(f"{name}: at least one slot and at most {MAX_SLOTS} per call (got {n})")
        return t, values

    @torch.compiler.disable
    def release(self, slots) -> None:
        """Give back the listed slots (a sequence of distinct ints in ``[0, B)`` or a 1-D int32 / int64 tensor on the device, whose distinctness
        is the caller's contract; indices outside ``[0, B)`` are skipped on the device): every entry a slot owns loses its reference and
        becomes -1, ``n_owned`` and ``lens`` of the slot become 0, and the pages whose last reference went in this call are pushed so that the
        lowest id among them is handed out next -- whatever the order of execution.  Two listed slots may share pages."""
        c = self.cache
        if isinstance(slots, (list, tuple)) and len(slots) == 0:
            raise ValueError("release: at least one slot and at most 1024 per call (got 0)")
        if isinstance(slots, (list, tuple)) and all(_is_int(s) for s in slots) and (any(not 0 <= s < c.B for s in slots) or len(set(slots)) != len(slots)):
            raise ValueError(f"slots must be distinct indices in [0, {c.B}) (got {list(slots)!r})")
        t, _ = self._slots("slots", slots, "slot indices")
        rc = _cabi_kvpool.load().sage_kvpool_release(*self._geometry(), _p(c.lens), _p(t), int(t.shape[0]), _stream(self.ws))
        _cabi.check(rc, "sage_kvpool_release")

    @torch.compiler.disable
    def fork(self, src_slots, dst_slots, prefix_lens=None):
        """:meth:`PagedQuantizedKVCache.fork` with the pool choosing the children's pages: ``fork_prepare`` adds a reference to every shared
        page, pops one page per child and writes ``dst_eff`` / ``new_pages`` on the device; ``cache.fork(src_slots, dst_eff, new_pages,
        prefix_lens)`` follows.  A fork is REFUSED -- ``dst_eff[i] = new_pages[i] = -1``, which the fork kernel skips entirely, and ``hdr``
        counts it -- when a slot index lies outside ``[0, B)``, source and destination are one, the destination still owns pages (release it
        first), or the pool is dry (the forks ``0 .. i`` that need a page ask for more than ``n_free``).  Arguments as there, without
        ``new_pages``.  Returns ``(dst_eff, new_pages)``, int32 ``[n]`` on the device."""
        c = self.cache
        if not c._seeded:
            raise ValueError("the cache has no statistics yet: seed(k_mean, v_amax) or from_prefill(...) before the first fork")
        for name, x in (("src_slots", src_slots), ("dst_slots", dst_slots)):
            if isinstance(x, (list, tuple)) and len(x) == 0:
                raise ValueError("src_slots, dst_slots and prefix_lens must have one length n >= 1 (got 0)")
        src, src_l = c._fork_index("src_slots", src_slots, c.B, "slot indices")
        dst, dst_l = c._fork_index("dst_slots", dst_slots, c.B, "slot indices")
        prefix = None if prefix_lens is None else c._fork_index("prefix_lens", prefix_lens, None, None)[0]
        n = int(src.shape[0])
        if n < 1 or any(t is not None and t.shape[0] != n for t in (dst, prefix)):
            raise ValueError(f"src_slots, dst_slots and prefix_lens must have one length n >= 1 (got {[int(t.shape[0]) for t in (src, dst, prefix) if t is not None]})")
        if n > MAX_SLOTS:
            raise ValueError(f"at most {MAX_SLOTS} forks per call (got {n})")
        if dst_l is not None and len(set(dst_l)) != n:
            raise ValueError(f"dst_slots must be distinct (got {dst_l!r})")
        if dst_l is not None and src_l is not None and set(dst_l) & set(src_l):
            raise ValueError(f"dst_slots must be disjoint from src_slots (got {src_l!r} -> {dst_l!r})")
        new_pages = torch.empty((n,), dtype=torch.int32, device=c.device)
        dst_eff = torch.empty((n,), dtype=torch.int32, device=c.device)
        rc = _cabi_kvpool.load().sage_kvpool_fork_prepare(*self._geometry(), _p(c.lens), _p(src), _p(dst), _p(prefix), n, _p(new_pages), _p(dst_eff), _stream(self.ws))
        _cabi.check(rc, "sage_kvpool_fork_prepare")
        c.fork(src, dst_eff, new_pages, prefix)
        return dst_eff, new_pages

    def status(self) -> dict:
        """THE host read: synchronises the current stream and returns ``n_free``, ``refused_last`` (slots or forks the last reserve / fork
        refused), ``pages_short`` (what that call lacked) and ``refused_total`` (since :meth:`init`)."""
        if self.ws.is_cuda:
            torch.cuda.current_stream(self.ws.device).synchronize()
        n_free, last, short, total = self.hdr[:4].tolist()
        return dict(n_free=n_free, refused_last=last, pages_short=short, refused_total=total)
