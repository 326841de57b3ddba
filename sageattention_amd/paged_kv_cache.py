"""The appendable quantised KV cache over a pool of pages, reached through a block table (gfx950 extension).

:class:`~sageattention_amd.kv_cache.QuantizedKVCache` keeps every sequence in one contiguous slab, so a serving caller reserves the longest
context it may ever see for every slot.  :class:`PagedQuantizedKVCache` keeps the same quantised operands in a POOL of ``num_pages`` pages of
``page_size = 64 * 2^k`` keys and a ``block_table`` the caller writes: logical 64-key tile ``t`` of sequence ``b`` lies in page
``block_table[b, t >> k]``, at tile ``t & (2^k - 1)`` of it.  The statistics are frozen as there, so a row's bytes depend on its own 64-key
block alone: the paged cache holds, at the places the table names, byte for byte what the contiguous cache holds, and
:func:`~sageattention_amd.kv_cache.sageattn_kvcache` -- which takes either cache -- returns bit for bit what it returns on the contiguous one.

Device rules: attention reads the table entries of tiles that hold a key it requests and no others, and clamps every id to
``[0, num_pages - 1]`` before it forms an address; an append does not write a block whose id lies outside ``[0, num_pages)`` (``lens`` still
advance).  A bad table gives wrong numbers, never an access outside the pool.  Two sequences that append into one page are the caller's error
and are not detected; there is no allocator here (:mod:`~sageattention_amd.paged_kv_pool` keeps one on the device, over a cache whose table it
alone writes).

Sequences share pages through :meth:`PagedQuantizedKVCache.fork`: the child's table names the parent's closed pages, the
parent's open page is copied into a page of the child's own, and the child takes the parent's frozen statistics -- which is what makes the
shared bytes exactly the child's own.

Only what paging adds is written here -- the pool's shapes, the block table, ``seed(slots=...)``, the C call of an append, ``fork``, the table
of ``from_prefill`` and what :func:`~sageattention_amd.kv_cache.sageattn_kvcache` asks a paged cache for; the rest is the base class of
:mod:`~sageattention_amd.kv_cache`, and the ``sage_kvpaged_attn`` call is a branch of ``core._attn_fused_q``.

Import from here (``from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache``); the names are not part of the package's
``__all__``.  Not under torch.compile.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _cabi, _cabi_kvfork, _cabi_kvpaged
from .kv_cache import _KVCacheBase, _is_int
from .quant import _dtype_code, _p, _stream

__all__ = ["PagedQuantizedKVCache"]


class PagedQuantizedKVCache(_KVCacheBase):
    """The quantised keys and values of ``B`` sequence slots of up to ``max_pages_per_seq * page_size`` tokens in a pool of ``num_pages`` pages.

    Public tensors, all on ``device``, shapes fixed at allocation.  The pool, laid out as a :class:`QuantizedKVCache` with ``B = num_pages``
    and ``capacity = page_size``: ``k_int8`` int8 ``[num_pages, Hkv, page_size, D]``; ``k_scale`` fp32 ``[num_pages, Hkv, page_size / 64 *
    4]``; ``v_image`` uint8 ``[num_pages, Hkv, page_size / 64, D, 64]``.  Per sequence slot: ``v_scale`` / ``v_amax`` fp32 ``[B, Hkv, D]``,
    ``k_mean`` ``[B, Hkv, D]`` in the input dtype (None after seeding without smoothing), ``k_tail`` / ``v_tail`` ``[B, Hkv, 64, D]``, ``lens``
    int32 ``[B]``.  ``block_table`` int32 ``[B, max_pages_per_seq]``: allocated here, filled with -1, written by the caller."""

    _paged = True

    def __init__(self, num_pages, page_size, B, max_pages_per_seq, Hkv, D, dtype, tensors):
        # (capacity: the logical capacity of a sequence, what Lk / capacity are to the contiguous cache)
        super().__init__(B, Hkv, max_pages_per_seq * page_size, D, dtype, tensors[:3], tensors[3:9])
        self.num_pages, self.page_size, self.max_pages_per_seq, self.block_table = num_pages, page_size, max_pages_per_seq, tensors[9]

    @classmethod
    def allocate(cls, num_pages: int, page_size: int, B: int, max_pages_per_seq: int, Hkv: int, D: int, dtype: torch.dtype, device) -> "PagedQuantizedKVCache":
        """An empty, unseeded cache.  Everything but ``lens`` (zero) and ``block_table`` (-1) is uninitialised memory: :meth:`seed` before the
        first append."""
        if not all(_is_int(x) for x in (num_pages, page_size, B, max_pages_per_seq, Hkv, D)) or min(num_pages, B, max_pages_per_seq, Hkv) < 1:
            raise ValueError(f"num_pages, page_size, B, max_pages_per_seq and Hkv must be positive ints (got {num_pages!r}, {page_size!r}, {B!r}, "
                             f"{max_pages_per_seq!r}, {Hkv!r})")
        if page_size < 64 or page_size & (page_size - 1):
            raise ValueError(f"page_size must be 64 * 2^k (got {page_size})")
        if max_pages_per_seq * page_size > 2 ** 30:
            raise ValueError(f"max_pages_per_seq * page_size must be at most 2^30 (got {max_pages_per_seq} * {page_size})")
        per_sequence = cls._per_sequence(B, Hkv, D, dtype, device)
        table = torch.full((B, max_pages_per_seq), -1, dtype=torch.int32, device=device)
        return cls(num_pages, page_size, B, max_pages_per_seq, Hkv, D, dtype, cls._store(num_pages, Hkv, page_size, D, device) + per_sequence + (table,))

    def _slot_index(self, slots) -> torch.Tensor:
        if isinstance(slots, torch.Tensor):
            if slots.dtype not in (torch.int32, torch.int64) or slots.dim() != 1 or slots.device != self.device:
                raise ValueError(f"slots must be a 1-D int32 / int64 tensor on {self.device} or a sequence of ints "
                                 f"(got {slots.dtype} {list(slots.shape)} on {slots.device})")
            return slots.to(torch.int64)
        if not isinstance(slots, (list, tuple)) or not all(_is_int(s) for s in slots):
            raise ValueError(f"slots must be a 1-D int32 / int64 tensor or a sequence of ints (got {slots!r})")
        if any(not 0 <= s < self.B for s in slots) or len(set(slots)) != len(slots):
            raise ValueError(f"slots must be distinct indices in [0, {self.B}) (got {list(slots)!r})")
        return torch.tensor(list(slots), dtype=torch.int64, device=self.device)

    def seed(self, k_mean: Optional[torch.Tensor], v_amax: torch.Tensor, slots=None) -> "PagedQuantizedKVCache":
        """Set the frozen statistics and empty the cache (``lens = 0``), as :meth:`QuantizedKVCache.seed` does.  ``slots`` (a sequence of ints
        or a 1-D index tensor on the device; indices of a tensor are the caller's to keep inside ``[0, B)`` and distinct) re-seeds ONLY those
        sequence slots -- the reuse of a slot a pool exists for: ``k_mean`` / ``v_amax`` are then ``[len(slots), Hkv, D]``, the cache must have
        been seeded as a whole before, and ``k_mean`` is None exactly if the cache's is (one attention call reads every slot's mean or
        none).  Device copies only; the block table and the pool are not touched, and neither is ``v_scale``: a re-seeded slot keeps its old
        ``v_scale`` row until the next append call writes every slot's from ``v_amax`` -- the call that gives the slot its first key, so no
        attention call reads the stale row to any effect (a slot without keys returns ``o = 0``, ``lse = -inf``)."""
        if slots is None:
            return self._seed(k_mean, v_amax)
        idx = self._slot_index(slots)
        if not self._seeded:
            raise ValueError("seed(slots=...) re-seeds slots of a seeded cache: seed(k_mean, v_amax) the whole cache first")
        if (k_mean is None) != (self.k_mean is None):
            raise ValueError(f"seed(slots=...): k_mean must be {'None' if self.k_mean is None else 'a tensor'} as the cache's is "
                             "(smoothing is one choice for every slot of a cache)")
        return self._seed(k_mean, v_amax, idx)

    @torch.compiler.disable
    def append(self, k_new: torch.Tensor, v_new: torch.Tensor, new_lens: Optional[torch.Tensor] = None, tensor_layout: str = "HND") -> None:
        """Append rows, as :meth:`QuantizedKVCache.append` does: a block goes to its place in the page ``block_table`` names when the launch
        runs.  Rows that do not fit into ``max_pages_per_seq * page_size`` are dropped on the device; a block whose page id lies outside
        ``[0, num_pages)`` is not written, and ``lens`` advance all the same.  Two launches on the current stream, no host read, no
        synchronisation: the call captures into a HIP graph and a replay follows the tensors' -- the table's included -- contents."""
        self._append(k_new, v_new, new_lens, tensor_layout)

    def _append_call(self, k_new, v_new, new_lens, T, k_strides, v_strides) -> None:
        rc = _cabi_kvpaged.load().sage_kvpaged_append(
            _p(self.k_int8), _p(self.k_scale), _p(self.v_image), _p(self.v_scale), _p(self.v_amax), _p(self.k_mean), _p(self.k_tail), _p(self.v_tail),
            _p(self.lens), _p(k_new), _p(v_new), _p(new_lens), self.B, self.Hkv, T, self.D, *k_strides, *v_strides, _dtype_code(k_new),
            _p(self.block_table), self.block_table.stride(0), self.num_pages, self.page_size, self.max_pages_per_seq, _stream(k_new))
        _cabi.check(rc, "sage_kvpaged_append")

    def _fork_index(self, name, x, limit, what):
        """One index argument of :meth:`fork` as (int32 tensor ``[n]`` on the device, the list of ints it was given as or None).  A sequence of
        ints is checked here (``limit``: the values lie in ``[0, limit)``; None: any int, clamped to int32); a tensor is never read."""
        if isinstance(x, torch.Tensor):
            if x.dtype not in (torch.int32, torch.int64) or x.dim() != 1 or x.device != self.device:
                raise ValueError(f"{name} must be a 1-D int32 / int64 tensor on {self.device} or a sequence of ints "
                                 f"(got {x.dtype} {list(x.shape)} on {x.device})")
            if x.dtype == torch.int64:
                x = x.clamp(-2 ** 31, 2 ** 31 - 1)
            return x.to(torch.int32).contiguous(), None
        if not isinstance(x, (list, tuple)) or not all(_is_int(s) for s in x):
            raise ValueError(f"{name} must be a 1-D int32 / int64 tensor or a sequence of ints (got {x!r})")
        if limit is not None and any(not 0 <= s < limit for s in x):
            raise ValueError(f"{name} must be {what} in [0, {limit}) (got {list(x)!r})")
        values = [max(-2 ** 31, min(2 ** 31 - 1, s)) for s in x]
        return torch.tensor(values, dtype=torch.int32, device=self.device), values

    @torch.compiler.disable
    def fork(self, src_slots, dst_slots, new_pages, prefix_lens=None) -> None:
        """Make sequence slot ``dst_slots[i]`` a copy of slot ``src_slots[i]`` that SHARES its closed pages, for ``n`` forks in one launch
        (``sage_kvfork``): one system prompt under many requests, ``n > 1`` samples of one prompt, beam search, a scratch copy to
        verify draft tokens on.  With ``L = clamp(lens[s], 0, capacity)`` and ``P = L`` (or, with ``prefix_lens``, ``P = clamp(prefix_lens[i],
        0, L)``), on the device:

        * ``block_table[d]`` takes the entries of ``block_table[s]`` for the ``P // page_size`` whole pages, as they stand, and behind them
          ``new_pages[i]`` -- the child's first own page (written whenever the table has an entry there, also when ``P`` ends on a page
          boundary: the child's next append goes there);
        * if ``P`` ends inside a page, the tiles of the parent's open page that hold keys are copied into ``new_pages[i]`` (copy-on-write;
          nothing of the pool is written when either id lies outside ``[0, num_pages)``, the append's rule);
        * ``v_scale`` / ``v_amax`` / ``k_mean``, the raw rows of the open 64-key block in ``k_tail`` / ``v_tail`` and ``lens`` of ``d`` become
          those of ``s`` (``lens[d] = P``).

        **A prefix shorter than the parent is rounded down to a multiple of 64 keys** (``P &= ~63`` when ``P < L``): only on a block boundary
        are the parent's bytes exactly the prefix's own -- its open block was quantised over more rows, and the raw rows of a closed block are
        gone.  The child takes the parent's frozen statistics, so every shared block is byte for byte what the child would have produced, and
        :func:`~sageattention_amd.kv_cache.sageattn_kvcache` on the child returns bit for bit what it returns on the parent; afterwards the
        two append independently.  A fork whose source or destination lies outside ``[0, B)``, or whose source is its destination, is skipped.

        ``src_slots`` / ``dst_slots`` / ``new_pages`` (and ``prefix_lens``, or None): each a 1-D int32 / int64 tensor on the cache's device
        (int64 is clamped and converted; never read on the host) or a sequence of ints, all of one length ``n >= 1``.  The contract:
        ``dst_slots`` are distinct and disjoint from ``src_slots`` (one source may fork to many destinations in one call); ``new_pages`` are
        distinct and named by no live table entry.  Sequences of ints are checked against it here, together with their ranges (ValueError);
        tensors are not -- a violation gives wrong numbers, never an access outside a tensor.  There is no allocator and there are no
        reference counts: which pages are free is the caller's to know.

        One launch on the current stream, no host read, no synchronisation: with tensor arguments the call captures into a HIP graph and a
        replay follows their, the lengths' and the table's contents."""
        if not self._seeded:
            raise ValueError("the cache has no statistics yet: seed(k_mean, v_amax) or from_prefill(...) before the first fork")
        src, src_l = self._fork_index("src_slots", src_slots, self.B, "slot indices")
        dst, dst_l = self._fork_index("dst_slots", dst_slots, self.B, "slot indices")
        pages, pages_l = self._fork_index("new_pages", new_pages, self.num_pages, "page ids")
        prefix = None if prefix_lens is None else self._fork_index("prefix_lens", prefix_lens, None, None)[0]
        n = int(src.shape[0])
        if n < 1 or any(t is not None and t.shape[0] != n for t in (dst, pages, prefix)):
            raise ValueError(f"src_slots, dst_slots, new_pages and prefix_lens must have one length n >= 1 "
                             f"(got {[int(t.shape[0]) for t in (src, dst, pages, prefix) if t is not None]})")
        if n > 65535:
            raise ValueError(f"at most 65535 forks per call (got {n})")
        if dst_l is not None and len(set(dst_l)) != n:
            raise ValueError(f"dst_slots must be distinct (got {dst_l!r})")
        if dst_l is not None and src_l is not None and set(dst_l) & set(src_l):
            raise ValueError(f"dst_slots must be disjoint from src_slots (got {src_l!r} -> {dst_l!r})")
        if pages_l is not None and len(set(pages_l)) != n:
            raise ValueError(f"new_pages must be distinct (got {pages_l!r})")
        rc = _cabi_kvfork.load().sage_kvfork(
            _p(self.k_int8), _p(self.k_scale), _p(self.v_image), _p(self.v_scale), _p(self.v_amax), _p(self.k_mean), _p(self.k_tail), _p(self.v_tail),
            _p(self.lens), _p(self.block_table), self.block_table.stride(0), self.num_pages, self.page_size, self.max_pages_per_seq,
            self.B, self.Hkv, self.D, _dtype_code(self.k_tail), _p(src), _p(dst), _p(pages), _p(prefix), n, _stream(self.k_int8))
        _cabi.check(rc, "sage_kvfork")

    @classmethod
    @torch.compiler.disable
    def from_prefill(cls, k: torch.Tensor, v: torch.Tensor, block_table: torch.Tensor, num_pages: int, page_size: int,
                     kv_lens: Optional[torch.Tensor] = None, tensor_layout: str = "HND", smooth_k: bool = True,
                     v_headroom: float = 2.0) -> "PagedQuantizedKVCache":
        """A cache seeded from a prompt's keys and values and filled with them through ``block_table`` (int32 / int64 ``[B,
        max_pages_per_seq]`` on the device, copied into the cache's own), statistics as :meth:`QuantizedKVCache.from_prefill` forms them."""
        B, H, L, D = cls._prefill_dims(k, v, tensor_layout, v_headroom)
        if not isinstance(block_table, torch.Tensor) or block_table.dtype not in (torch.int32, torch.int64) or block_table.dim() != 2 or \
                block_table.shape[0] != B or block_table.shape[1] < 1 or block_table.device != k.device:
            raise ValueError(f"block_table must be an int32 or int64 tensor [B, max_pages_per_seq] = [{B}, >= 1] on {k.device}")
        cache = cls.allocate(num_pages, page_size, B, int(block_table.shape[1]), H, D, k.dtype, k.device)
        if cache.capacity < L:
            raise ValueError(f"block_table's {block_table.shape[1]} pages of {page_size} keys do not hold the prefill's {L} rows")
        lens = cls._prefill_lens(kv_lens, B, L, k.device)
        cache.block_table.copy_(block_table.clamp(-2 ** 31, 2 ** 31 - 1) if block_table.dtype == torch.int64 else block_table)
        return cache._prefill(k, v, lens, tensor_layout, smooth_k, v_headroom)

    # ---- what sageattn_kvcache asks a cache for ----
    def _k_logical(self, tensor_layout):
        # (the resolver reads K's shape alone: the logical [B, Hkv, capacity, D], without memory)
        shape = (self.B, self.Hkv, self.capacity, self.D) if tensor_layout == "HND" else (self.B, self.capacity, self.Hkv, self.D)
        return torch.empty(shape, dtype=torch.int8, device="meta")

    def _refuse_keywords(self, num_splits) -> None:
        if num_splits is not None:
            raise ValueError(f"num_splits is not supported on a PagedQuantizedKVCache (got {num_splits!r}): the split's first pass and its kernels "
                             "do not look pages up; pass None")
