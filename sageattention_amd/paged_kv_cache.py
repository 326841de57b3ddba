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
and are not detected; there is no allocator here.

Only what paging adds is written here -- the pool's shapes, the block table, ``seed(slots=...)``, the C call of an append, the table of
``from_prefill`` and what :func:`~sageattention_amd.kv_cache.sageattn_kvcache` asks a paged cache for; the rest is the base class of
:mod:`~sageattention_amd.kv_cache`, and the ``sage_kvpaged_attn`` call is a branch of ``core._attn_fused_q``.

Import from here (``from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache``); the names are not part of the package's
``__all__``.  Not under torch.compile.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _cabi, _cabi_kvpaged
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
        none).  Device copies only; the block table and the pool are not touched."""
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
