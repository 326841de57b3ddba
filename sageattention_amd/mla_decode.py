"""FP8-PV attention for the absorbed multi-head-latent-attention decode shape (gfx950): ``sageattn_mla_decode`` and ``mla_quantize_latent``.

After prefill the DeepSeek-V2 / V3 / R1 line attends in the absorbed form: all query heads read one shared latent row of 576 channels per token
(512 compressed + 64 rope), and V is the first 512 channels of that same row.  ``sageattn`` stops at 128 channels, ``sageattn_hd256`` at 256,
``sageattn_qk192`` at 192 / 128, and none of them lets V be a slice of K.  This module is the arithmetic of the default FP8 route -- K smoothed by
its per-channel mean, per-thread INT8 K, INT8 Q with one scale per query row, the exact score form, e4m3 V with a per-channel scale at
``scale_max = 448``, two-level FP32 accumulation -- on kernels written for 576 / 512 (include/sage_mla_gfx950.h).  The import path
is ``sageattention_amd.mla_decode``; the package's ``__all__`` is the reference's list and stays so.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Union

import torch

from . import _cabi, _cabi_mla, _cabi_mlasplit
from .core import _finish
from .quant import _aligned, _p, _stream

WIDTH_QK, WIDTH_V = 576, 512


@dataclass(frozen=True)
class MlaLatent:
    """A latent cache quantised once by :func:`mla_quantize_latent`: the private images and statistics of include/sage_mla_gfx950.h."""
    k_img: torch.Tensor        # [B, ntile, 36864] uint8
    v_img: torch.Tensor        # [B, ntile, 32768] uint8
    k_scale: torch.Tensor      # [B, 4 ntile] fp32
    v_scale: torch.Tensor      # [B, 512] fp32
    k_mean: torch.Tensor       # [B, 576] in the dtype of kv
    kv_lens: Optional[torch.Tensor]
    smooth_k: bool
    Lk: int


def _redirect(width: int, what: str) -> str:
    if width <= 128:
        return f"{what}: call sageattention_amd.sageattn for head_dim <= 128"
    if width <= 192:
        return f"{what}: call sageattention_amd.qk192.sageattn_qk192 for 192-wide q / k against 128-wide v"
    if width <= 256:
        return f"{what}: call sageattention_amd.hd256.sageattn_hd256 for head_dim <= 256"
    return f"{what}: there is no other entry for this width"


def _check_kv(kv, kv_lens, name):
    if torch.compiler.is_compiling():
        raise ValueError(f"{name} is not supported under torch.compile: call it from eager code (torch.compiler.disable)")
    if not isinstance(kv, torch.Tensor) or kv.dim() != 3:
        raise ValueError(f"{name}: kv must be 3-D [B, Lk, 576], one shared latent row per token "
                         f"(got {tuple(kv.shape) if isinstance(kv, torch.Tensor) else type(kv).__name__})")
    if kv.size(-1) != WIDTH_QK:
        raise ValueError(_redirect(kv.size(-1), f"{name} takes latent rows of 576 channels, 512 compressed + 64 rope (got {kv.size(-1)})"))
    if kv.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"{name}: kv must be torch.float16 or torch.bfloat16 (got {kv.dtype}): cast with .half() / .bfloat16()")
    if kv_lens is not None and (not isinstance(kv_lens, torch.Tensor) or kv_lens.dtype != torch.int32 or kv_lens.dim() != 1
                                or kv_lens.numel() != kv.size(0)):
        raise ValueError(f"{name}: kv_lens must be an int32 tensor of shape [{kv.size(0)}] (one length per sample): cast with .to(torch.int32)")
    if not kv.is_cuda:
        raise ValueError(f"{name} needs kv on a CUDA (ROCm) device: move it with .cuda(); there is no CPU path")
    if kv.size(0) < 1 or kv.size(1) < 1:
        raise ValueError(f"{name}: kv needs at least one sample and one row (got {tuple(kv.shape)})")
    if kv.stride(-1) != 1:
        raise ValueError("Last dim of kv must be contiguous: call .contiguous()")
    if kv_lens is not None and (kv_lens.device != kv.device or not kv_lens.is_contiguous()):
        raise ValueError(f"{name}: kv_lens must be contiguous on the device of kv ({kv.device}); the call never reads it on the host")


def mla_quantize_latent(kv: torch.Tensor, kv_lens: Optional[torch.Tensor] = None, smooth_k: bool = True) -> MlaLatent:
    """Quantise the latent cache ``kv [B, Lk, 576]`` (fp16 / bf16) once: the INT8 K image of all 576 channels (smoothed by the per-channel mean
    over each sample's valid rows) and the e4m3 V image of ``kv[..., :512]``.  ``kv_lens`` (int32 ``[B]`` on the device, default ``Lk``) is the
    number of valid rows of each sample; rows from there on are never read.  Nothing synchronises with the host.  The result goes to
    :func:`sageattn_mla_decode` in place of ``kv``, step after step."""
    _check_kv(kv, kv_lens, "mla_quantize_latent")
    torch.cuda.set_device(kv.device)
    kv = _aligned(kv, 8)
    lib = _cabi_mla.load()
    B, Lk, dev = kv.size(0), kv.size(1), kv.device
    ntile = (Lk + 63) // 64
    k_img = torch.empty((B, ntile, 64 * WIDTH_QK), dtype=torch.uint8, device=dev)
    v_img = torch.empty((B, ntile, 64 * WIDTH_V), dtype=torch.uint8, device=dev)
    k_scale = torch.empty((B, 4 * ntile), dtype=torch.float32, device=dev)
    v_scale = torch.empty((B, WIDTH_V), dtype=torch.float32, device=dev)
    k_mean = torch.empty((B, WIDTH_QK), dtype=kv.dtype, device=dev)
    ws_floats = lib.sage_mla_ws_floats(B, Lk)
    ws = torch.empty((ws_floats,), dtype=torch.float32, device=dev)
    code = _cabi.DTYPE_F16 if kv.dtype == torch.float16 else _cabi.DTYPE_BF16
    rc = lib.sage_mla_prepass(_p(kv), _p(kv_lens), _p(k_img), _p(k_scale), _p(k_mean), _p(v_img), _p(v_scale), _p(ws), ws_floats, B, Lk,
                              WIDTH_QK, WIDTH_V, kv.stride(0), kv.stride(1), int(bool(smooth_k)), code, _stream(kv))
    _cabi.check(rc, "sage_mla_prepass")
    return MlaLatent(k_img, v_img, k_scale, v_scale, k_mean, kv_lens, bool(smooth_k), Lk)


# The "auto" plan's constants, read off profiles/mla_split_probe.json (tools/mla_split_probe.py; bf16, Hq 128, Lq 1 / 2, B 1 .. 128, Lk 4096 ..
# 32768): with W = B * ceil(rows / 128) work items the fastest S measured is the power of two that brings S * W to about one workgroup per CU
# (W 1 .. 8 -> 32, 16 -> 16, 32 -> 8, 64 -> 4, 128 -> 2; x0.08 .. x0.88 of the unsplit launch, spreads <= 0.03), and at W = 256 every S is slower
# than the unsplit launch.  Nothing below Lk 4096 was measured.
_AUTO_MIN_LK, _AUTO_WORKGROUPS, _AUTO_MAX_SPLITS, _AUTO_MAX_ITEMS = 4096, 256, 32, 128


def _auto_num_splits(B: int, rows: int, Lk: int) -> int:
    """The ``num_splits="auto"`` plan, from shapes only: the number of chunks for ``B * ceil(rows / 128)`` work items against ``Lk`` keys, or 1
    for the unsplit launch -- which it is wherever the probe did not show the split faster by more than both spreads."""
    items = B * ((rows + 127) // 128)
    if Lk < _AUTO_MIN_LK or items > _AUTO_MAX_ITEMS:
        return 1
    S = min(_AUTO_MAX_SPLITS, _AUTO_WORKGROUPS // items)
    return 1 << (S.bit_length() - 1)


def _resolve_num_splits(num_splits, name: str) -> int:
    """``num_splits`` as an int: 1 the unsplit launch, 2 .. 255 that many chunks, 0 the plan from the shapes."""
    if num_splits is None:
        return 1
    if torch.compiler.is_compiling():
        raise ValueError(f"{name}: num_splits is not supported under torch.compile: call it from eager code (torch.compiler.disable)")
    if isinstance(num_splits, str) and num_splits == "auto":
        return 0
    if isinstance(num_splits, int) and not isinstance(num_splits, bool) and 0 <= num_splits <= 255:
        return num_splits
    raise ValueError(f"{name}: num_splits must be None or 1 (one workgroup per sample and 128-row block), an int from 2 to 255 (that many "
                     f"key-range chunks, exactly the unsplit arithmetic) or 'auto' / 0 (got {num_splits!r})")


def sageattn_mla_decode(q: torch.Tensor, kv: Union[torch.Tensor, MlaLatent], kv_lens: Optional[torch.Tensor] = None,
                        sm_scale: Optional[float] = None, smooth_k: bool = True, return_lse: bool = False, num_splits=None):
    """INT8 QK^T + FP8 (e4m3) PV attention of ``q [B, Lq, Hq, 576]`` (last dim contiguous, any strides in front) against the latent cache
    ``kv [B, Lk, 576]`` with V = ``kv[..., :512]``: ``o [B, Lq, Hq, 512]`` in the dtype of ``q``, with ``return_lse`` also the natural-log LSE
    ``[B, Hq, Lq]`` in fp32.  The mask is the decode one: query position i of sample b sees key j iff ``j <= kv_lens[b] - Lq + i``
    (``kv_lens`` int32 ``[B]`` on the device, default ``Lk``); a position in front of key 0 gives ``o = +0``, ``lse = -inf``.  ``Lq = 1`` is the
    plain decode step, ``Lq = 2 .. 8`` multi-token prediction.  ``sm_scale`` defaults to ``576 ** -0.5``.  ``kv`` may be the result of
    :func:`mla_quantize_latent`, which skips the pre-pass (``kv_lens`` and ``smooth_k`` are then the quantised state's); the two ways are bit
    for bit the same.  ``num_splits=S`` (2 .. 255) runs every work item as S key-range chunks on S times as many workgroups, exactly: every
    e4m3 P is the unsplit call's, only the FP32 summation order of O and l differs; it is for small batches against long
    latents, where the unsplit launch fills a fraction of the chip.  ``None`` / 1 is the unsplit launch, ``"auto"`` / 0 a plan from the
    shapes.  Nothing synchronises with the host.  Everything else raises ``ValueError`` and names the entry to call."""
    name = "sageattn_mla_decode"
    S = _resolve_num_splits(num_splits, name)
    if isinstance(kv, MlaLatent):
        if torch.compiler.is_compiling():
            raise ValueError(f"{name} is not supported under torch.compile: call it from eager code (torch.compiler.disable)")
        if kv_lens is not None and kv_lens is not kv.kv_lens:
            raise ValueError(f"{name}: the quantised latent carries its own kv_lens; quantise again for other lengths")
        lat = kv
    else:
        _check_kv(kv, kv_lens, name)
        lat = None
    like = lat.k_mean if lat is not None else kv
    if not isinstance(q, torch.Tensor) or q.dim() != 4:
        raise ValueError(f"{name}: q must be 4-D [B, Lq, Hq, 576] (got {tuple(q.shape) if isinstance(q, torch.Tensor) else type(q).__name__})")
    if q.size(-1) != WIDTH_QK:
        raise ValueError(_redirect(q.size(-1), f"{name} takes query rows of 576 channels (got {q.size(-1)})"))
    if q.dtype != like.dtype:
        raise ValueError(f"{name}: q and kv must share one dtype, torch.float16 or torch.bfloat16 (got {q.dtype} and {like.dtype})")
    if not q.is_cuda or q.device != like.device:
        raise ValueError(f"{name} needs q and kv on one CUDA (ROCm) device: move them with .cuda(); there is no CPU path")
    if q.size(0) != like.size(0) or q.size(1) < 1 or q.size(2) < 1:
        raise ValueError(f"{name}: q must have the batch of kv and at least one position and head (got q {tuple(q.shape)}, batch {like.size(0)})")
    if q.stride(-1) != 1:
        raise ValueError("Last dim of q must be contiguous: call .contiguous()")
    if lat is None:
        lat = mla_quantize_latent(kv, kv_lens, smooth_k)
    torch.cuda.set_device(q.device)
    if sm_scale is None:
        sm_scale = WIDTH_QK ** -0.5
    q = _aligned(q, 8)
    lib = _cabi_mla.load()
    B, Lq, Hq, _ = q.shape
    o = torch.empty((B, Lq, Hq, WIDTH_V), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, Hq, Lq), dtype=torch.float32, device=q.device) if return_lse else None
    code = _cabi.DTYPE_F16 if q.dtype == torch.float16 else _cabi.DTYPE_BF16
    args = (_p(q), _p(lat.k_img), _p(lat.v_img), _p(lat.k_scale), _p(lat.v_scale), _p(lat.kv_lens), _p(o), _p(lse), B, Lq, Hq, lat.Lk, WIDTH_QK,
            WIDTH_V, q.stride(0), q.stride(1), q.stride(2), float(sm_scale), code, _stream(q))
    if S == 0:
        S = _auto_num_splits(B, Lq * Hq, lat.Lk)
    if S == 1:
        _cabi.check(lib.sage_mla_attn(*args), "sage_mla_attn")
    else:
        split = _cabi_mlasplit.load()
        ws_bytes = split.sage_mlasplit_ws_bytes(B, Lq, Hq, S)
        if ws_bytes < 0:
            _cabi.check(-1, "sage_mlasplit_ws_bytes")
        ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=q.device)      # chunk_max, lse_part, o_part: sized from the shapes alone
        _cabi.check(split.sage_mlasplit_attn(*args, S, _p(ws), ws_bytes), "sage_mlasplit_attn")
    lse_correction = None
    if return_lse and lat.smooth_k:
        # q . mean per row in FP32 over the 576 channels (the product's rounding to bf16 would cost the LSE close to 1e-2), [B, Hq, Lq]
        lse_correction = (q.float() * lat.k_mean[:, None, None, :].float()).sum(-1).transpose(1, 2)
    return _finish(o, lse, WIDTH_V, return_lse, lat.smooth_k, lse_correction, sm_scale)
