"""An appendable quantised KV cache for decode on the FP8-PV ``kv_lens`` kernels (gfx950 extension).

``sageattn_qk_int8_pv_fp8_cuda(q, k, v, kv_lens=...)`` runs the whole K / V pre-pass -- K mean, INT8 K, FP8 V image -- over the whole
context on every call, to add one token.  :class:`QuantizedKVCache` keeps the operands that the attention entry
``sage_attn_fused_q_pv_f8_kvlens`` takes and appends rows to them in place (``sage_kvcache_append``: two small launches, no host read, graph
capturable); :func:`sageattn_kvcache` attends a query to it through that entry with ``Lk = capacity`` and ``kv_lens = cache.lens``.  No
attention kernel knows about the cache.

The statistics are frozen when the cache is seeded: the K mean (softmax does not change when a constant vector is subtracted from every
key, so any mean is exact and the LSE correction works with it) and the per-channel V abs-max the FP8 conversion divides by (e4m3 is
floating point: head-room costs no relative precision above the subnormal range; values beyond it saturate at the format's largest finite
value, as in the pre-pass).  Seeded with the statistics of its final content, a cache holds byte for byte what the pre-pass produces from
that content, whatever the schedule of appends, and :func:`sageattn_kvcache` returns bit for bit what the one-shot call returns.

What this cache and the paged one (:mod:`~sageattention_amd.paged_kv_cache`) have in common lives here once, in the private base class
:class:`_KVCacheBase`: the per-sequence tensors, seeding, the checks of appended rows, ``append`` up to the C call, the pieces of
``from_prefill``, and what :func:`sageattn_kvcache` asks a cache for.  A subclass adds where its keys lie and its one C call.

Import from here (``from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache``); the names are not part of the package's
``__all__``.  Not under torch.compile.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _cabi, _cabi_kvcache, core
from .quant import _aligned, _dims, _dtype_code, _p, _stream, channel_mean_kvlens

__all__ = ["QuantizedKVCache", "sageattn_kvcache"]


def _layout_ok(tensor_layout) -> None:
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


class _KVCacheBase:
    """The quantised keys and values of ``B`` sequences of up to ``capacity`` tokens, wherever the keys lie: the per-sequence tensors
    (``v_scale`` / ``v_amax`` fp32 ``[B, Hkv, D]``, ``k_mean`` ``[B, Hkv, D]`` and ``k_tail`` / ``v_tail`` ``[B, Hkv, 64, D]`` in the input
    dtype, ``lens`` int32 ``[B]``) and the store ``k_int8`` / ``k_scale`` / ``v_image``, whose shapes are the subclass's."""

    def __init__(self, B, Hkv, capacity, D, dtype, store, per_sequence):
        self.B, self.Hkv, self.capacity, self.D, self.dtype = B, Hkv, capacity, D, dtype
        self.k_int8, self.k_scale, self.v_image = store
        self.v_scale, self.v_amax, self.k_mean, self.k_tail, self.v_tail, self.lens = per_sequence
        self._k_mean_buf = self.k_mean
        self._seeded = False

    @property
    def device(self) -> torch.device:
        return self.k_int8.device

    # ---- allocation ----
    @classmethod
    def _per_sequence(cls, B, Hkv, D, dtype, device):
        """The ``D`` / ``dtype`` errors of ``allocate`` and the six per-sequence tensors (``lens`` zero, the rest uninitialised)."""
        if D not in (64, 128):
            raise ValueError(f"Unsupported head_dim: {D} (a {cls.__name__} takes 64 or 128)")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"dtype must be torch.float16 or torch.bfloat16 (got {dtype})")
        f32 = dict(dtype=torch.float32, device=device)
        return (torch.empty((B, Hkv, D), **f32), torch.empty((B, Hkv, D), **f32), torch.empty((B, Hkv, D), dtype=dtype, device=device),
                torch.empty((B, Hkv, 64, D), dtype=dtype, device=device), torch.empty((B, Hkv, 64, D), dtype=dtype, device=device),
                torch.zeros((B,), dtype=torch.int32, device=device))

    @staticmethod
    def _store(n, Hkv, rows, D, device):
        """``k_int8`` / ``k_scale`` / ``v_image`` of ``n`` slabs (or pages) of ``rows`` keys each, uninitialised."""
        return (torch.empty((n, Hkv, rows, D), dtype=torch.int8, device=device),
                torch.empty((n, Hkv, rows // 64 * 4), dtype=torch.float32, device=device),
                torch.empty((n, Hkv, rows // 64, D, 64), dtype=torch.uint8, device=device))

    # ---- seeding ----
    def _seed(self, k_mean, v_amax, idx=None):
        """``seed`` of the whole cache, or (``idx``: an int64 index tensor) of those sequences alone: the checks, then device copies."""
        shape = (self.B if idx is None else idx.shape[0], self.Hkv, self.D)
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

    # ---- appending ----
    def _new_rows(self, k_new, v_new, tensor_layout):
        """The argument errors of rows offered to the cache."""
        _layout_ok(tensor_layout)
        for name, t in (("k_new", k_new), ("v_new", v_new)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4:
                raise ValueError(f"{name} must be a 4-D tensor (got {type(t).__name__} {list(getattr(t, 'shape', ()))})")
            if t.dtype != self.dtype:
                raise ValueError(f"{name} must have the cache's dtype {self.dtype} (got {t.dtype})")
            if t.device != self.device:
                raise ValueError(f"{name} must be on the cache's device {self.device} (got {t.device})")
        if k_new.shape != v_new.shape:
            raise ValueError(f"k_new and v_new must have one shape (got {list(k_new.shape)}, {list(v_new.shape)})")
        B, H, T, D = _dims(k_new, tensor_layout)[:4]
        if (B, H, D) != (self.B, self.Hkv, self.D):
            raise ValueError(f"new rows must have B, Hkv, D = {self.B}, {self.Hkv}, {self.D} (got {B}, {H}, {D}; layout {tensor_layout})")
        if T < 1:
            raise ValueError("new rows: at least one row per call (T >= 1)")

    def _append(self, k_new, v_new, new_lens, tensor_layout) -> None:
        """``append``: every argument error, ``new_lens`` as int32, the rows aligned, then the subclass's one C call (``_append_call``)."""
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
        T = _dims(k_new, tensor_layout)[2]
        self._append_call(k_new, v_new, new_lens, T, _dims(k_new, tensor_layout)[4:], _dims(v_new, tensor_layout)[4:])

    # ---- the pieces of from_prefill ----
    @staticmethod
    def _prefill_dims(k, v, tensor_layout, v_headroom):
        """The errors of ``from_prefill``'s ``tensor_layout`` / ``k`` / ``v`` / ``v_headroom``; (B, Hkv, L, D) of the prompt."""
        _layout_ok(tensor_layout)
        if not isinstance(k, torch.Tensor) or not isinstance(v, torch.Tensor) or k.dim() != 4 or k.shape != v.shape or k.dtype != v.dtype or k.device != v.device:
            raise ValueError("k and v must be 4-D tensors of one shape, dtype and device")
        if isinstance(v_headroom, bool) or not isinstance(v_headroom, (int, float)) or not 0.0 < float(v_headroom) < float("inf"):
            raise ValueError(f"v_headroom must be a positive finite number (got {v_headroom!r})")
        B, H, L, D = _dims(k, tensor_layout)[:4]
        if L < 1:
            raise ValueError("from_prefill needs at least one row")
        return B, H, L, D

    @staticmethod
    def _prefill_lens(kv_lens, B, L, device):
        """The valid rows per sample of a prompt of ``L`` rows, int32 ``[B]`` on the device (``kv_lens`` None: all)."""
        if kv_lens is None:
            return torch.full((B,), L, dtype=torch.int32, device=device)
        if not isinstance(kv_lens, torch.Tensor) or kv_lens.dtype not in (torch.int32, torch.int64) or kv_lens.shape != (B,) or kv_lens.device != device:
            raise ValueError(f"kv_lens must be an int32 or int64 tensor [B] = [{B}] on {device}")
        return kv_lens.clamp(0, L).to(torch.int32).contiguous()

    def _prefill(self, k, v, lens, tensor_layout, smooth_k, v_headroom):
        """Seed from the prompt's valid rows (torch ops on the device, no synchronisation) and append them all."""
        B, _, L = _dims(k, tensor_layout)[:3]
        seq = 2 if tensor_layout == "HND" else 1
        valid = torch.arange(L, device=k.device).unsqueeze(0) < lens.unsqueeze(1)                       # [B, L]
        valid = valid.view(B, 1, L, 1) if tensor_layout == "HND" else valid.view(B, L, 1, 1)
        v_amax = torch.where(valid, v.abs().to(torch.float32), 0.0).amax(dim=seq) * float(v_headroom)   # [B, H, D]; padding rows may hold anything
        self.seed(channel_mean_kvlens(k, lens, tensor_layout) if smooth_k else None, v_amax)
        self.append(k, v, lens, tensor_layout)
        return self

    # ---- what sageattn_kvcache asks a cache for ----
    _paged = False          # the store is a pool of pages behind ``block_table``: the attention call is ``sage_kvpaged_attn``

    def _k_operand(self, tensor_layout):
        """The INT8 K of the attention call in the caller's layout (head-major storage, as the pre-pass's; the strides are the kernel's)."""
        return self.k_int8 if tensor_layout == "HND" else self.k_int8.permute(0, 2, 1, 3)

    def _k_logical(self, tensor_layout):
        """What the keyword resolver reads K's shape from: ``[B, Hkv, capacity, D]`` in the caller's layout."""
        return self._k_operand(tensor_layout)

    def _refuse_keywords(self, num_splits) -> None:
        """The keywords this kind of cache does not take, refused before the family's resolver sees them."""


class QuantizedKVCache(_KVCacheBase):
    """The quantised keys and values of ``B`` sequences of up to ``capacity`` tokens, ``Hkv`` kv-heads, head size ``D`` (64 or 128).

    Public tensors, all on ``device``, shapes fixed at allocation (``capacity`` rounded up to a multiple of 64):

    ``k_int8``  int8 ``[B, Hkv, capacity, D]``; ``k_scale`` fp32 ``[B, Hkv, capacity / 64 * 4]``; ``v_image`` uint8 ``[B, Hkv, capacity / 64,
    D, 64]`` (the FP8 tile image); ``v_scale`` fp32 ``[B, Hkv, D]``; ``v_amax`` fp32 ``[B, Hkv, D]`` and ``k_mean`` ``[B, Hkv, D]`` in the
    input dtype (the frozen statistics; ``k_mean`` is None after seeding without smoothing); ``k_tail`` / ``v_tail`` ``[B, Hkv, 64, D]`` in the
    input dtype (the raw rows of each sample's open 64-key block); ``lens`` int32 ``[B]``."""

    def __init__(self, B, Hkv, capacity, D, dtype, tensors):
        super().__init__(B, Hkv, capacity, D, dtype, tensors[:3], tensors[3:])

    @classmethod
    def allocate(cls, B: int, Hkv: int, capacity: int, D: int, dtype: torch.dtype, device) -> "QuantizedKVCache":
        """An empty, unseeded cache.  Everything but ``lens`` (zero) is uninitialised memory: :meth:`seed` before the first append."""
        if not all(_is_int(x) for x in (B, Hkv, capacity, D)) or B < 1 or Hkv < 1 or capacity < 1:
            raise ValueError(f"B, Hkv and capacity must be positive ints (got {B!r}, {Hkv!r}, {capacity!r})")
        per_sequence = cls._per_sequence(B, Hkv, D, dtype, device)
        cap = (capacity + 63) // 64 * 64
        return cls(B, Hkv, cap, D, dtype, cls._store(B, Hkv, cap, D, device) + per_sequence)

    def seed(self, k_mean: Optional[torch.Tensor], v_amax: torch.Tensor) -> "QuantizedKVCache":
        """Set the frozen statistics and empty the cache (``lens = 0``).  ``k_mean``: ``[B, Hkv, D]`` in the cache's dtype, or None for no
        smoothing; ``v_amax``: ``[B, Hkv, D]``, the per-channel abs-max the FP8 conversion uses (converted to fp32).  Device copies only."""
        return self._seed(k_mean, v_amax)

    @torch.compiler.disable
    def append(self, k_new: torch.Tensor, v_new: torch.Tensor, new_lens: Optional[torch.Tensor] = None, tensor_layout: str = "HND") -> None:
        """Append rows: ``k_new`` / ``v_new`` ``[B, Hkv, T, D]`` (HND) or ``[B, T, Hkv, D]`` (NHD) in the cache's dtype; sample b takes the first
        ``new_lens[b]`` of them (int32 / int64 ``[B]`` on the device, clamped there to ``[0, T]``; None: all T).  Rows that do not fit into
        ``capacity`` are dropped on the device.  Rows at or behind ``new_lens[b]`` are never read.  Two launches on the current stream, no
        host read, no synchronisation: the call captures into a HIP graph and a replay follows the tensors' contents."""
        self._append(k_new, v_new, new_lens, tensor_layout)

    def _append_call(self, k_new, v_new, new_lens, T, k_strides, v_strides) -> None:
        rc = _cabi_kvcache.load().sage_kvcache_append(
            _p(self.k_int8), _p(self.k_scale), _p(self.v_image), _p(self.v_scale), _p(self.v_amax), _p(self.k_mean), _p(self.k_tail), _p(self.v_tail),
            _p(self.lens), _p(k_new), _p(v_new), _p(new_lens), self.B, self.Hkv, self.capacity, T, self.D,
            *k_strides, *v_strides, _dtype_code(k_new), _stream(k_new))
        _cabi.check(rc, "sage_kvcache_append")

    @classmethod
    @torch.compiler.disable
    def from_prefill(cls, k: torch.Tensor, v: torch.Tensor, capacity: int, kv_lens: Optional[torch.Tensor] = None, tensor_layout: str = "HND",
                     smooth_k: bool = True, v_headroom: float = 2.0) -> "QuantizedKVCache":
        """A cache seeded from a prompt's keys and values and filled with them: ``k_mean = channel_mean_kvlens(k, lens)`` (None without
        ``smooth_k``), ``v_amax = v_headroom * max|v|`` per channel over the valid rows (torch ops on the device, no synchronisation), then one
        append of all rows.  ``kv_lens``: int32 / int64 ``[B]`` on the device, the valid rows per sample (None: all)."""
        B, H, L, D = cls._prefill_dims(k, v, tensor_layout, v_headroom)
        cache = cls.allocate(B, H, capacity, D, k.dtype, k.device)
        if cache.capacity < L:
            raise ValueError(f"capacity {capacity} does not hold the prefill's {L} rows")
        return cache._prefill(k, v, cls._prefill_lens(kv_lens, B, L, k.device), tensor_layout, smooth_k, v_headroom)


def _attend(name, q, cache, tensor_layout, is_causal, causal_align, q_start, window_size, pack_gqa, num_splits, sm_scale, return_lse,
            paged_split: bool):
    """What :func:`sageattn_kvcache` and :func:`~sageattention_amd.paged_kv_split.sageattn_kvcache_split` do (``name``: the caller's, for the
    messages).  ``paged_split``: a paged cache takes ``num_splits`` (the second name) instead of refusing it (the first)."""
    if torch.compiler.is_compiling():
        raise ValueError(f"{name} is not supported under torch.compile")
    if not isinstance(cache, _KVCacheBase):
        raise ValueError(f"cache must be a QuantizedKVCache or a PagedQuantizedKVCache (got {type(cache).__name__})")
    _layout_ok(tensor_layout)
    if not isinstance(q, torch.Tensor) or q.dim() != 4:
        raise ValueError(f"q must be a 4-D tensor (got {type(q).__name__} {list(getattr(q, 'shape', ()))})")
    if q.dtype != cache.dtype:
        raise ValueError(f"q must have the cache's dtype {cache.dtype} (got {q.dtype})")
    if q.device != cache.device:
        raise ValueError(f"q must be on the cache's device {cache.device} (got {q.device})")
    B, Hq, Lq, D = _dims(q, tensor_layout)[:4]
    if B != cache.B or D != cache.D:
        raise ValueError(f"q must have B, D = {cache.B}, {cache.D} (got {B}, {D}; layout {tensor_layout})")
    if Hq % cache.Hkv != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by the cache's num_kv_heads ({cache.Hkv})")
    if q.stride(-1) != 1:
        raise ValueError("Last dim of q must be contiguous.")
    if not cache._seeded:
        raise ValueError("the cache has no statistics yet: seed(k_mean, v_amax) or from_prefill(...) first")
    if not paged_split:
        cache._refuse_keywords(num_splits)
    # the keywords' checks and meanings are sageattn_qk_int8_pv_fp8_cuda's: one resolver (no kv_lens keyword here; the route's fixed options)
    call = core._kv_family_args(q, cache._k_logical(tensor_layout), tensor_layout, is_causal, None, q_start, causal_align, window_size, pack_gqa,
                                num_splits, "per_thread", "fp32+fp16", False, {})
    torch.cuda.set_device(q.device)
    if sm_scale is None:
        sm_scale = D ** -0.5
    smooth_k = cache.k_mean is not None
    lse_correction = None
    if smooth_k and return_lse:
        lse_correction = core._lse_correction(q, cache.k_mean.unsqueeze(1 if tensor_layout == "NHD" else 2), tensor_layout)
    return core._attn_kv_family(call, q, cache.lens, cache.lens, cache._k_operand(tensor_layout), cache.v_image, cache.v_scale, cache.k_scale,
                                tensor_layout, sm_scale, return_lse, D, smooth_k, lse_correction, paged=cache if cache._paged else None)


@torch.compiler.disable
def sageattn_kvcache(q: torch.Tensor, cache, tensor_layout: str = "HND", is_causal: bool = False, causal_align: str = "top_left",
                     q_start=None, window_size=None, pack_gqa=False, num_splits=None, sm_scale: Optional[float] = None, return_lse: bool = False):
    """Attention of ``q`` (``[B, Hq, Lq, D]`` HND / ``[B, Lq, Hq, D]`` NHD, the cache's dtype) to the cache's first ``cache.lens[b]`` keys per
    sample: ``sageattn_qk_int8_pv_fp8_cuda(q, k, v, kv_lens=cache.lens, ...)`` without its pre-pass.  ``is_causal``, ``causal_align``,
    ``q_start``, ``window_size``, ``pack_gqa``, ``num_splits``, ``sm_scale`` and ``return_lse`` mean what they mean there and raise the same
    ValueErrors; the padded key length of the call is ``cache.capacity``.  Nothing reads the lengths on the host.

    ``cache`` may also be a :class:`~sageattention_amd.paged_kv_cache.PagedQuantizedKVCache`: the same call through its block table
    (``sage_kvpaged_attn``), bit for bit the result on a contiguous cache of the same content; ``num_splits`` other than None is refused
    there (:func:`~sageattention_amd.paged_kv_split.sageattn_kvcache_split` takes it)."""
    return _attend("sageattn_kvcache", q, cache, tensor_layout, is_causal, causal_align, q_start, window_size, pack_gqa, num_splits, sm_scale,
                   return_lse, False)
