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

Import from here (``from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache``); the names are not part of the package's
``__all__``.  Not under torch.compile.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _cabi, _cabi_kvpaged, core, ops
from .kv_cache import QuantizedKVCache, _layout_ok
from .quant import _aligned, _dims, _dtype_code, _p, _stream, channel_mean_kvlens

__all__ = ["PagedQuantizedKVCache"]


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


class PagedQuantizedKVCache:
    """The quantised keys and values of ``B`` sequence slots of up to ``max_pages_per_seq * page_size`` tokens in a pool of ``num_pages`` pages.

    Public tensors, all on ``device``, shapes fixed at allocation.  The pool, laid out as a :class:`QuantizedKVCache` with ``B = num_pages``
    and ``capacity = page_size``: ``k_int8`` int8 ``[num_pages, Hkv, page_size, D]``; ``k_scale`` fp32 ``[num_pages, Hkv, page_size / 64 *
    4]``; ``v_image`` uint8 ``[num_pages, Hkv, page_size / 64, D, 64]``.  Per sequence slot: ``v_scale`` / ``v_amax`` fp32 ``[B, Hkv, D]``,
    ``k_mean`` ``[B, Hkv, D]`` in the input dtype (None after seeding without smoothing), ``k_tail`` / ``v_tail`` ``[B, Hkv, 64, D]``, ``lens``
    int32 ``[B]``.  ``block_table`` int32 ``[B, max_pages_per_seq]``: allocated here, filled with -1, written by the caller."""

    def __init__(self, num_pages, page_size, B, max_pages_per_seq, Hkv, D, dtype, tensors):
        self.num_pages, self.page_size, self.B, self.max_pages_per_seq, self.Hkv, self.D, self.dtype = num_pages, page_size, B, max_pages_per_seq, Hkv, D, dtype
        self.capacity = max_pages_per_seq * page_size        # the logical capacity of a sequence: what Lk / capacity are to the contiguous cache
        (self.k_int8, self.k_scale, self.v_image, self.v_scale, self.v_amax, self.k_mean, self.k_tail, self.v_tail, self.lens, self.block_table) = tensors
        self._k_mean_buf = self.k_mean
        self._seeded = False

    @property
    def device(self) -> torch.device:
        return self.k_int8.device

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
        if D not in (64, 128):
            raise ValueError(f"Unsupported head_dim: {D} (a PagedQuantizedKVCache takes 64 or 128)")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"dtype must be torch.float16 or torch.bfloat16 (got {dtype})")
        device = torch.device(device)
        f32 = dict(dtype=torch.float32, device=device)
        tensors = (torch.empty((num_pages, Hkv, page_size, D), dtype=torch.int8, device=device),
                   torch.empty((num_pages, Hkv, page_size // 64 * 4), **f32),
                   torch.empty((num_pages, Hkv, page_size // 64, D, 64), dtype=torch.uint8, device=device),
                   torch.empty((B, Hkv, D), **f32),
                   torch.empty((B, Hkv, D), **f32),
                   torch.empty((B, Hkv, D), dtype=dtype, device=device),
                   torch.empty((B, Hkv, 64, D), dtype=dtype, device=device),
                   torch.empty((B, Hkv, 64, D), dtype=dtype, device=device),
                   torch.zeros((B,), dtype=torch.int32, device=device),
                   torch.full((B, max_pages_per_seq), -1, dtype=torch.int32, device=device))
        return cls(num_pages, page_size, B, max_pages_per_seq, Hkv, D, dtype, tensors)

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
        n = self.B
        idx = None
        if slots is not None:
            idx = self._slot_index(slots)
            n = idx.shape[0]
            if not self._seeded:
                raise ValueError("seed(slots=...) re-seeds slots of a seeded cache: seed(k_mean, v_amax) the whole cache first")
            if (k_mean is None) != (self.k_mean is None):
                raise ValueError(f"seed(slots=...): k_mean must be {'None' if self.k_mean is None else 'a tensor'} as the cache's is "
                                 "(smoothing is one choice for every slot of a cache)")
        shape = (n, self.Hkv, self.D)
        if k_mean is not None:
            if not isinstance(k_mean, torch.Tensor) or tuple(k_mean.shape) != shape or k_mean.dtype != self.dtype or k_mean.device != self.device:
                raise ValueError(f"k_mean must be a {self.dtype} tensor {list(shape)} on {self.device} or None "
                                 f"(got {getattr(k_mean, 'dtype', type(k_mean).__name__)} {list(getattr(k_mean, 'shape', ()))})")
        if not isinstance(v_amax, torch.Tensor) or tuple(v_amax.shape) != shape or not v_amax.dtype.is_floating_point or v_amax.device != self.device:
            raise ValueError(f"v_amax must be a floating-point tensor {list(shape)} on {self.device} "
                             f"(got {getattr(v_amax, 'dtype', type(v_amax).__name__)} {list(getattr(v_amax, 'shape', ()))})")
        if idx is not None:
            if k_mean is not None:
                self.k_mean.index_copy_(0, idx, k_mean)
            self.v_amax.index_copy_(0, idx, v_amax.to(torch.float32))
            self.lens.index_fill_(0, idx, 0)
            return self
        if k_mean is None:
            self.k_mean = None
        else:
            self.k_mean = self._k_mean_buf
            self.k_mean.copy_(k_mean)
        self.v_amax.copy_(v_amax)
        self.lens.zero_()
        self._seeded = True
        return self

    _new_rows = QuantizedKVCache._new_rows

    @torch.compiler.disable
    def append(self, k_new: torch.Tensor, v_new: torch.Tensor, new_lens: Optional[torch.Tensor] = None, tensor_layout: str = "HND") -> None:
        """Append rows, as :meth:`QuantizedKVCache.append` does: a block goes to its place in the page ``block_table`` names when the launch
        runs.  Rows that do not fit into ``max_pages_per_seq * page_size`` are dropped on the device; a block whose page id lies outside
        ``[0, num_pages)`` is not written, and ``lens`` advance all the same.  Two launches on the current stream, no host read, no
        synchronisation: the call captures into a HIP graph and a replay follows the tensors' -- the table's included -- contents."""
        if not self._seeded:
            raise ValueError("the cache has no statistics yet: seed(k_mean, v_amax) or from_prefill(...) before the first append")
        self._new_rows(k_new, v_new, tensor_layout)
        if new_lens is not None:
            if not isinstance(new_lens, torch.Tensor) or new_lens.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"new_lens must be an int32 or int64 tensor (got {getattr(new_lens, 'dtype', type(new_lens).__name__)})")
            if new_lens.dim() != 1 or new_lens.shape[0] != self.B:
                raise ValueError(f"new_lens must have shape [B] = [{self.B}] (got {tuple(new_lens.shape)})")
            if new_lens.device != self.device:
                raise ValueError(f"new_lens must be on the cache's device {self.device} (got {new_lens.device})")
            if new_lens.dtype == torch.int64:
                new_lens = new_lens.clamp(-2 ** 31, 2 ** 31 - 1)
            new_lens = new_lens.to(torch.int32).contiguous()
        k_new, v_new = _aligned(k_new, 8), _aligned(v_new, 8)
        _, _, T, _, k_sb, k_sh, k_sl = _dims(k_new, tensor_layout)
        _, _, _, _, v_sb, v_sh, v_sl = _dims(v_new, tensor_layout)
        rc = _cabi_kvpaged.load().sage_kvpaged_append(
            _p(self.k_int8), _p(self.k_scale), _p(self.v_image), _p(self.v_scale), _p(self.v_amax), _p(self.k_mean), _p(self.k_tail), _p(self.v_tail),
            _p(self.lens), _p(k_new), _p(v_new), _p(new_lens), self.B, self.Hkv, T, self.D,
            k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, _dtype_code(k_new),
            _p(self.block_table), self.block_table.stride(0), self.num_pages, self.page_size, self.max_pages_per_seq, _stream(k_new))
        _cabi.check(rc, "sage_kvpaged_append")

    @classmethod
    @torch.compiler.disable
    def from_prefill(cls, k: torch.Tensor, v: torch.Tensor, block_table: torch.Tensor, num_pages: int, page_size: int,
                     kv_lens: Optional[torch.Tensor] = None, tensor_layout: str = "HND", smooth_k: bool = True,
                     v_headroom: float = 2.0) -> "PagedQuantizedKVCache":
        """A cache seeded from a prompt's keys and values and filled with them through ``block_table`` (int32 / int64 ``[B,
        max_pages_per_seq]`` on the device, copied into the cache's own), statistics as :meth:`QuantizedKVCache.from_prefill` forms them."""
        _layout_ok(tensor_layout)
        if not isinstance(k, torch.Tensor) or not isinstance(v, torch.Tensor) or k.dim() != 4 or k.shape != v.shape or k.dtype != v.dtype or k.device != v.device:
            raise ValueError("k and v must be 4-D tensors of one shape, dtype and device")
        if isinstance(v_headroom, bool) or not isinstance(v_headroom, (int, float)) or not 0.0 < float(v_headroom) < float("inf"):
            raise ValueError(f"v_headroom must be a positive finite number (got {v_headroom!r})")
        B, H, L, D = _dims(k, tensor_layout)[:4]
        if L < 1:
            raise ValueError("from_prefill needs at least one row")
        if not isinstance(block_table, torch.Tensor) or block_table.dtype not in (torch.int32, torch.int64) or block_table.dim() != 2 or \
                block_table.shape[0] != B or block_table.shape[1] < 1 or block_table.device != k.device:
            raise ValueError(f"block_table must be an int32 or int64 tensor [B, max_pages_per_seq] = [{B}, >= 1] on {k.device}")
        cache = cls.allocate(num_pages, page_size, B, int(block_table.shape[1]), H, D, k.dtype, k.device)
        if cache.capacity < L:
            raise ValueError(f"block_table's {block_table.shape[1]} pages of {page_size} keys do not hold the prefill's {L} rows")
        if kv_lens is None:
            lens = torch.full((B,), L, dtype=torch.int32, device=k.device)
        else:
            if not isinstance(kv_lens, torch.Tensor) or kv_lens.dtype not in (torch.int32, torch.int64) or kv_lens.shape != (B,) or kv_lens.device != k.device:
                raise ValueError(f"kv_lens must be an int32 or int64 tensor [B] = [{B}] on {k.device}")
            lens = kv_lens.clamp(0, L).to(torch.int32).contiguous()
        cache.block_table.copy_(block_table.clamp(-2 ** 31, 2 ** 31 - 1) if block_table.dtype == torch.int64 else block_table)
        seq = 2 if tensor_layout == "HND" else 1
        valid = torch.arange(L, device=k.device).unsqueeze(0) < lens.unsqueeze(1)                       # [B, L]
        valid = valid.view(B, 1, L, 1) if tensor_layout == "HND" else valid.view(B, L, 1, 1)
        v_amax = torch.where(valid, v.abs().to(torch.float32), 0.0).amax(dim=seq) * float(v_headroom)   # [B, H, D]; padding rows may hold anything
        cache.seed(channel_mean_kvlens(k, lens, tensor_layout) if smooth_k else None, v_amax)
        cache.append(k, v, lens, tensor_layout)
        return cache


def _attend(q: torch.Tensor, cache: PagedQuantizedKVCache, tensor_layout, is_causal, causal_align, q_start, window_size, pack_gqa, num_splits,
            sm_scale, return_lse):
    """``sageattn_kvcache`` on a paged cache, behind its checks of ``q`` against the cache: the keywords through the family's one resolver (same
    ValueErrors, same order), then ``sage_kvpaged_attn``."""
    if num_splits is not None:
        raise ValueError(f"num_splits is not supported on a PagedQuantizedKVCache (got {num_splits!r}): the split's first pass and its kernels "
                         "do not look pages up; pass None")
    B, Hq, Lq, D, q_sb, q_sh, q_sl = _dims(q, tensor_layout)
    # (the resolver reads K's shape alone: the logical [B, Hkv, capacity, D], without memory)
    k_shape = torch.empty((B, cache.Hkv, cache.capacity, D) if tensor_layout == "HND" else (B, cache.capacity, cache.Hkv, D), dtype=torch.int8, device="meta")
    call = core._kv_family_args(q, k_shape, tensor_layout, is_causal, None, q_start, causal_align, window_size, pack_gqa, None,
                                "per_thread", "fp32+fp16", False, {})
    torch.cuda.set_device(q.device)
    if sm_scale is None:
        sm_scale = D ** -0.5
    smooth_k = cache.k_mean is not None
    lse_correction = None
    if smooth_k and return_lse:
        lse_correction = core._lse_correction(q, cache.k_mean.unsqueeze(1 if tensor_layout == "NHD" else 2), tensor_layout)
    start = core._q_start_tensor(call.q_start, cache.lens, B, Lq, cache.capacity, q.device, call.shift) if call.with_start else None
    q = _aligned(q, 8)
    B, Hq, Lq, D, q_sb, q_sh, q_sl = _dims(q, tensor_layout)
    k_pool = cache.k_int8 if tensor_layout == "HND" else cache.k_int8.permute(0, 2, 1, 3)      # (head-major storage; the strides are the kernel's)
    _, _, _, _, k_sb, k_sh, k_sl = _dims(k_pool, tensor_layout)
    o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    _, _, _, _, o_sb, o_sh, o_sl = _dims(o, tensor_layout)
    lse = torch.empty((B, Hq, Lq), dtype=torch.float32, device=q.device) if return_lse else None
    code = _cabi.DTYPE_F16 if q.dtype == torch.float16 else _cabi.DTYPE_BF16
    h = ops._hooks
    attr = _cabi.launch_attr(grid_out=h.grid_probe, q_start=start, window=call.window, gqa_pack=call.gqa_pack)      # (no launch workspace: the ordinary dispatch)
    rc = _cabi_kvpaged.load().sage_kvpaged_attn(
        _p(q), _p(cache.k_int8), _p(cache.v_image), _p(o), _p(lse), _p(cache.k_scale), _p(cache.v_scale), _p(cache.lens),
        _p(cache.block_table), cache.block_table.stride(0), cache.num_pages, cache.page_size, cache.max_pages_per_seq,
        B, Hq, cache.Hkv, Lq, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, o_sb, o_sh, o_sl,
        int(call.is_causal), float(core._sm_log2(sm_scale)), code, code, _stream(q), _cabi.attr_arg(attr))
    _cabi.check(rc, "sage_kvpaged_attn")
    return core._finish(o, lse, D, return_lse, smooth_k, lse_correction, sm_scale)
