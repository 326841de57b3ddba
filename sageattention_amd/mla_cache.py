"""An appendable quantised latent for the absorbed MLA decode call (gfx950): :class:`MlaLatentCache`.

``sageattn_mla_decode(q, kv, kv_lens)`` runs the three-launch pre-pass over the whole latent on every call, and ``mla_quantize_latent`` freezes
a latent that nothing can add a token to.  :class:`MlaLatentCache` keeps the operands the attention entries take and appends rows to them in
place (``sage_mlacache_append``: two small launches, no host read, graph capturable).  Attention is the existing call:
``sageattn_mla_decode(q, cache.latent(), num_splits=...)`` -- :meth:`MlaLatentCache.latent` is an :class:`~sageattention_amd.mla_decode.MlaLatent`
whose tensors are the cache's own, whose ``kv_lens`` is ``cache.lens`` and whose ``Lk`` is the capacity, so one ``latent()`` serves every step.

The statistics are frozen when the cache is seeded: the K mean (softmax does not change when one vector is subtracted from every key, so any
mean is exact and the LSE correction works with it) and the per-channel V abs-max the e4m3 conversion divides by (floating point: head-room
costs no relative precision above the subnormal range; values beyond it saturate at +-448).  Seeded with the statistics of its final content, a
cache holds byte for byte what ``mla_quantize_latent`` makes of that content, whatever the schedule of appends, and the attention call returns
bit for bit what it returns on the one-shot latent.

Import from here (``from sageattention_amd.mla_cache import MlaLatentCache``); the name is not part of the package's ``__all__``.  Not under
torch.compile.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _cabi, _cabi_mla, _cabi_mlacache
from .mla_decode import WIDTH_QK, WIDTH_V, MlaLatent, _check_kv, _redirect
from .quant import _aligned, _p, _stream

__all__ = ["MlaLatentCache"]


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


class MlaLatentCache:
    """The quantised latent of ``B`` sequences of up to ``capacity`` tokens.

    Public tensors, all on ``device``, shapes fixed at allocation (``ntile = ceil(capacity / 64)``): ``k_img`` uint8 ``[B, ntile, 36864]``,
    ``v_img`` uint8 ``[B, ntile, 32768]``, ``k_scale`` fp32 ``[B, 4 ntile]``, ``v_scale`` fp32 ``[B, 512]`` (the attention operands);
    ``k_mean`` ``[B, 576]`` in ``dtype`` and ``v_amax`` fp32 ``[B, 512]`` (the frozen statistics); ``lens`` int32 ``[B]`` (zeros); ``tail``
    ``[B, 64, 576]`` in ``dtype`` (the raw rows of each sample's open 64-key tile).  Everything but ``lens`` is uninitialised until
    :meth:`seed` (or :meth:`from_prefill`) and the appends that follow."""

    def __init__(self, B: int, capacity: int, dtype: torch.dtype, device, smooth_k: bool = True):
        if not _is_int(B) or not _is_int(capacity) or B < 1 or capacity < 1:
            raise ValueError(f"MlaLatentCache: B and capacity must be positive ints (got {B!r}, {capacity!r})")
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"MlaLatentCache: dtype must be torch.float16 or torch.bfloat16 (got {dtype})")
        self.B, self.capacity, self.dtype, self.smooth_k = B, capacity, dtype, bool(smooth_k)
        ntile = (capacity + 63) // 64
        u8, f32 = dict(dtype=torch.uint8, device=device), dict(dtype=torch.float32, device=device)
        self.k_img = torch.empty((B, ntile, 64 * WIDTH_QK), **u8)
        self.v_img = torch.empty((B, ntile, 64 * WIDTH_V), **u8)
        self.k_scale = torch.empty((B, 4 * ntile), **f32)
        self.v_scale = torch.empty((B, WIDTH_V), **f32)
        self.k_mean = torch.empty((B, WIDTH_QK), dtype=dtype, device=device)
        self.v_amax = torch.empty((B, WIDTH_V), **f32)
        self.lens = torch.zeros((B,), dtype=torch.int32, device=device)
        self.tail = torch.empty((B, 64, WIDTH_QK), dtype=dtype, device=device)
        self._seeded = False
        self._latent = MlaLatent(self.k_img, self.v_img, self.k_scale, self.v_scale, self.k_mean, self.lens, self.smooth_k, capacity)

    @property
    def device(self) -> torch.device:
        return self.k_img.device

    def latent(self) -> MlaLatent:
        """The cache as the operand of ``sageattn_mla_decode``: the cache's own tensors, ``kv_lens = lens``, ``Lk = capacity``.  It follows
        every later append; nothing is copied."""
        if not self._seeded:
            raise ValueError("MlaLatentCache.latent: the cache has no statistics yet: seed(k_mean, v_amax) or from_prefill(...) first")
        return self._latent

    def seed(self, k_mean: Optional[torch.Tensor], v_amax: torch.Tensor) -> "MlaLatentCache":
        """Set the frozen statistics and empty the cache (``lens = 0``).  ``k_mean``: ``[B, 576]`` in the cache's dtype (ignored, and stored as
        zeros, without ``smooth_k``; None is zeros too); ``v_amax``: floating point ``[B, 512]``, the per-channel abs-max the e4m3 conversion
        divides by (converted to fp32).  Device copies only."""
        if k_mean is not None and (not isinstance(k_mean, torch.Tensor) or tuple(k_mean.shape) != (self.B, WIDTH_QK)
                                   or k_mean.dtype != self.dtype or k_mean.device != self.device):
            raise ValueError(f"MlaLatentCache.seed: k_mean must be a {self.dtype} tensor [{self.B}, 576] on {self.device} or None "
                             f"(got {getattr(k_mean, 'dtype', type(k_mean).__name__)} {list(getattr(k_mean, 'shape', ()))})")
        if (not isinstance(v_amax, torch.Tensor) or tuple(v_amax.shape) != (self.B, WIDTH_V) or not v_amax.dtype.is_floating_point
                or v_amax.device != self.device):
            raise ValueError(f"MlaLatentCache.seed: v_amax must be a floating-point tensor [{self.B}, 512] on {self.device} "
                             f"(got {getattr(v_amax, 'dtype', type(v_amax).__name__)} {list(getattr(v_amax, 'shape', ()))})")
        if k_mean is None or not self.smooth_k:
            self.k_mean.zero_()
        else:
            self.k_mean.copy_(k_mean)
        self.v_amax.copy_(v_amax)
        self.lens.zero_()
        self._seeded = True
        return self

    def _check_rows(self, kv_new, name):
        """The refusals of rows offered to the cache, in the style (and order) of ``mla_decode._check_kv``."""
        if torch.compiler.is_compiling():
            raise ValueError(f"{name} is not supported under torch.compile: call it from eager code (torch.compiler.disable)")
        if not isinstance(kv_new, torch.Tensor) or kv_new.dim() != 3:
            raise ValueError(f"{name}: kv_new must be 3-D [B, T, 576], one latent row per token "
                             f"(got {tuple(kv_new.shape) if isinstance(kv_new, torch.Tensor) else type(kv_new).__name__})")
        if kv_new.size(-1) != WIDTH_QK:
            raise ValueError(_redirect(kv_new.size(-1), f"{name} takes latent rows of 576 channels, 512 compressed + 64 rope "
                                                        f"(got {kv_new.size(-1)})"))
        if kv_new.dtype != self.dtype:
            raise ValueError(f"{name}: kv_new must have the cache's dtype {self.dtype} (got {kv_new.dtype})")
        if kv_new.device != self.device:
            raise ValueError(f"{name}: kv_new must be on the cache's device {self.device} (got {kv_new.device})")
        if kv_new.size(0) != self.B or kv_new.size(1) < 1:
            raise ValueError(f"{name}: kv_new needs the cache's batch {self.B} and at least one row (got {tuple(kv_new.shape)})")
        if kv_new.stride(-1) != 1:
            raise ValueError("Last dim of kv_new must be contiguous: call .contiguous()")

    def append(self, kv_new: torch.Tensor, new_lens: Optional[torch.Tensor] = None) -> None:
        """Append rows: ``kv_new [B, T, 576]`` in the cache's dtype (last dim contiguous); sample b takes the first ``new_lens[b]`` of them (int32
        ``[B]`` on the device, clamped there to ``[0, T]``; None: all T).  Rows that do not fit into ``capacity`` are dropped on the device; rows
        at or behind ``new_lens[b]`` are never read.  Two launches on the current stream, no host read, no synchronisation: the call captures
        into a HIP graph, and a replay follows the contents of ``kv_new``, ``new_lens`` and ``lens``."""
        name = "MlaLatentCache.append"
        self._check_rows(kv_new, name)
        if not self._seeded:
            raise ValueError(f"{name}: the cache has no statistics yet: seed(k_mean, v_amax) or from_prefill(...) before the first append")
        if new_lens is not None and (not isinstance(new_lens, torch.Tensor) or new_lens.dtype != torch.int32 or new_lens.dim() != 1
                                     or new_lens.numel() != self.B or new_lens.device != self.device or not new_lens.is_contiguous()):
            raise ValueError(f"{name}: new_lens must be a contiguous int32 tensor of shape [{self.B}] on {self.device}: cast with "
                             f".to(torch.int32); the call never reads it on the host")
        torch.cuda.set_device(self.device)
        kv_new = _aligned(kv_new, 8)
        code = _cabi.DTYPE_F16 if self.dtype == torch.float16 else _cabi.DTYPE_BF16
        rc = _cabi_mlacache.load().sage_mlacache_append(
            _p(kv_new), _p(new_lens), _p(self.lens), _p(self.tail), _p(self.k_mean), _p(self.v_amax), _p(self.k_img), _p(self.k_scale),
            _p(self.v_img), _p(self.v_scale), self.B, kv_new.size(1), self.capacity, kv_new.stride(0), kv_new.stride(1), int(self.smooth_k),
            code, _stream(kv_new))
        _cabi.check(rc, "sage_mlacache_append")

    @classmethod
    def from_prefill(cls, kv: torch.Tensor, kv_lens: Optional[torch.Tensor] = None, capacity: Optional[int] = None, v_headroom: float = 2.0,
                     smooth_k: bool = True) -> "MlaLatentCache":
        """A cache seeded from a prompt ``kv [B, Lk, 576]`` and filled with it.  The statistics of each sample's valid rows (``kv_lens`` int32
        ``[B]`` on the device, default ``Lk``) are taken on the device by the pre-pass's own statistics kernels (``sage_mlacache_stats``);
        ``v_amax`` is multiplied by ``v_headroom``; then the prompt goes through :meth:`append`, the one quantising path.  A sample whose prompt
        is empty gets zero statistics -- every V byte it appends would be zero -- and needs :meth:`seed` before it is used.  ``capacity``
        defaults to ``Lk``.  Nothing synchronises with the host."""
        name = "MlaLatentCache.from_prefill"
        _check_kv(kv, kv_lens, name)
        if isinstance(v_headroom, bool) or not isinstance(v_headroom, (int, float)) or not 0.0 < float(v_headroom) < float("inf"):
            raise ValueError(f"{name}: v_headroom must be a positive finite number (got {v_headroom!r})")
        B, Lk = kv.size(0), kv.size(1)
        capacity = Lk if capacity is None else capacity
        if not _is_int(capacity) or capacity < Lk:
            raise ValueError(f"{name}: capacity {capacity!r} does not hold the prompt's {Lk} rows")
        cache = cls(B, capacity, kv.dtype, kv.device, smooth_k)
        torch.cuda.set_device(kv.device)
        kv = _aligned(kv, 8)
        ws_floats = _cabi_mla.load().sage_mla_ws_floats(B, Lk)
        ws = torch.empty((ws_floats,), dtype=torch.float32, device=kv.device)
        code = _cabi.DTYPE_F16 if kv.dtype == torch.float16 else _cabi.DTYPE_BF16
        rc = _cabi_mlacache.load().sage_mlacache_stats(_p(kv), _p(kv_lens), _p(cache.k_mean), _p(cache.v_amax), _p(ws), ws_floats, B, Lk,
                                                       kv.stride(0), kv.stride(1), int(cache.smooth_k), code, _stream(kv))
        _cabi.check(rc, "sage_mlacache_stats")
        cache.v_amax.mul_(float(v_headroom))
        cache._seeded = True
        cache.append(kv, kv_lens)
        return cache
