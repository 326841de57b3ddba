"""FP8-PV attention for head dimensions above 128, up to 256 (gfx950): ``sageattn_hd256``.

``sageattn`` and every other entry of the package stop at ``head_dim = 128``, as the reference does.  This module is the arithmetic of the
default FP8 route -- ``sageattn_qk_int8_pv_fp8_cuda`` with its defaults: K smoothed by its per-channel mean, per-thread INT8 Q and K, the
exact score form, e4m3 V with a per-channel scale at ``scale_max = 448``, two-level FP32 accumulation -- on kernels written for
``head_dim = 256`` (include/sage_hd256_gfx950.h).  The import path is ``sageattention_amd.hd256``; the package's ``__all__`` is the
reference's list and stays so.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import _cabi, _cabi_hd256
from .core import _finish
from .quant import _aligned, _dims, _p, _stream

HEAD_DIM = 256


def _check(q, k, v, tensor_layout):
    if torch.compiler.is_compiling():
        raise ValueError("sageattn_hd256 is not supported under torch.compile: call it from eager code (torch.compiler.disable)")
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")
    if not (q.dim() == k.dim() == v.dim() == 4):
        raise ValueError(f"q, k, v must be 4-D (got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})")
    d = q.size(-1)
    if d <= 128:
        raise ValueError(f"sageattn_hd256 takes 128 < head_dim <= 256 (got {d}): call sageattention_amd.sageattn for head_dim <= 128")
    if d > HEAD_DIM:
        raise ValueError(f"Unsupported head_dim: {d} (sageattn_hd256 takes 128 < head_dim <= 256; split the heads, or call "
                         "torch.nn.functional.scaled_dot_product_attention)")
    if not (q.is_cuda and k.is_cuda and v.is_cuda and q.device == k.device == v.device):
        raise ValueError("sageattn_hd256 needs q, k and v on one CUDA (ROCm) device: move them with .cuda(); there is no CPU path")
    if q.dtype not in (torch.float16, torch.bfloat16) or not (q.dtype == k.dtype == v.dtype):
        raise ValueError(f"q, k, v must share one dtype, torch.float16 or torch.bfloat16 (got {q.dtype}, {k.dtype}, {v.dtype}): cast with .half() / .bfloat16()")
    qB, qH, _, qD = _dims(q, tensor_layout)[:4]
    kd, vd = _dims(k, tensor_layout)[:4], _dims(v, tensor_layout)[:4]
    if kd != vd or (qB, qD) != (kd[0], kd[3]):
        raise ValueError(f"k and v must have one shape and agree with q in batch and head_dim (got q {tuple(q.shape)}, k {tuple(k.shape)}, "
                         f"v {tuple(v.shape)}, layout {tensor_layout})")
    if qH % kd[1] != 0:
        raise ValueError(f"num_qo_heads ({qH}) must be divisible by num_kv_heads ({kd[1]})")
    if _dims(q, tensor_layout)[2] < 1 or kd[2] < 1:
        raise ValueError("qo_len and kv_len must be at least 1")
    if not (q.stride(-1) == k.stride(-1) == v.stride(-1) == 1):
        raise ValueError("Last dim of qkv must be contiguous: call .contiguous()")


def sageattn_hd256(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tensor_layout: str = "HND", is_causal: bool = False,
                   sm_scale: Optional[float] = None, smooth_k: bool = True, return_lse: bool = False):
    """INT8 QK^T + FP8 (e4m3) PV attention for ``128 < head_dim <= 256``; head dims below 256 are zero-padded to 256 and the output is
    sliced back.  fp16 / bf16 inputs in "HND" or "NHD" layout, GQA (``Hq % Hkv == 0``), any ``qo_len >= 1`` and ``kv_len >= 1``, top-left
    causal.  ``sm_scale`` defaults to ``head_dim ** -0.5`` of the head_dim given.  ``return_lse`` as for ``sageattn_qk_int8_pv_fp8_cuda``:
    ``(o, lse)`` with the natural-log LSE ``[B, Hq, qo_len]``.  Everything else -- ``head_dim <= 128`` (``sageattn``), ``head_dim > 256``, a
    wrong dtype or device, mismatched shapes, use under torch.compile -- raises ``ValueError``."""
    _check(q, k, v, tensor_layout)
    torch.cuda.set_device(q.device)
    head_dim_og = q.size(-1)
    if sm_scale is None:
        sm_scale = head_dim_og ** -0.5
    if head_dim_og < HEAD_DIM:
        q, k, v = (F.pad(t, (0, HEAD_DIM - head_dim_og)) for t in (q, k, v))
    q, k, v = _aligned(q, 8), _aligned(k, 8), _aligned(v, 8)
    lib = _cabi_hd256.load()
    B, Hq, Lq, D, q_sb, q_sh, q_sl = _dims(q, tensor_layout)
    _, Hkv, Lk, _, k_sb, k_sh, k_sl = _dims(k, tensor_layout)
    _, _, _, _, v_sb, v_sh, v_sl = _dims(v, tensor_layout)
    dev = q.device
    ntile = (Lk + 63) // 64
    code = _cabi.DTYPE_F16 if q.dtype == torch.float16 else _cabi.DTYPE_BF16
    k_img = torch.empty((B, Hkv, ntile, 64 * D), dtype=torch.uint8, device=dev)
    v_img = torch.empty((B, Hkv, ntile, 64 * D), dtype=torch.uint8, device=dev)
    k_scale = torch.empty((B, Hkv, 4 * ntile), dtype=torch.float32, device=dev)
    v_scale = torch.empty((B, Hkv, D), dtype=torch.float32, device=dev)
    k_mean = torch.empty((B, Hkv, D), dtype=q.dtype, device=dev)
    ws_floats = lib.sage_hd256_ws_floats(B, Hkv, Lk)
    ws = torch.empty((ws_floats,), dtype=torch.float32, device=dev)
    rc = lib.sage_hd256_prepass(_p(k), _p(v), _p(k_img), _p(k_scale), _p(k_mean), _p(v_img), _p(v_scale), _p(ws), ws_floats, B, Hkv, Lk, D,
                                k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, int(bool(smooth_k)), code, _stream(q))
    _cabi.check(rc, "sage_hd256_prepass")
    o = torch.empty(q.shape, dtype=q.dtype, device=dev)
    _, _, _, _, o_sb, o_sh, o_sl = _dims(o, tensor_layout)
    lse = torch.empty((B, Hq, Lq), dtype=torch.float32, device=dev) if return_lse else None
    rc = lib.sage_hd256_attn(_p(q), _p(k_img), _p(v_img), _p(k_scale), _p(v_scale), _p(o), _p(lse), B, Hq, Hkv, Lq, Lk, D,
                             q_sb, q_sh, q_sl, o_sb, o_sh, o_sl, int(bool(is_causal)), float(sm_scale), code, _stream(q))
    _cabi.check(rc, "sage_hd256_attn")
    lse_correction = None
    if return_lse and smooth_k:
        km = k_mean.unsqueeze(1 if tensor_layout == "NHD" else 2)      # [B, 1, Hkv, D] / [B, Hkv, 1, D]: k.mean(dim=seq, keepdim=True)
        # q . km^T per row in FP32 (at 256 channels the product's rounding to bf16 would cost the LSE 1e-2), km broadcast over the GQA group
        nh = 2 if tensor_layout == "NHD" else 1
        lse_correction = (q.float() * torch.repeat_interleave(km, Hq // Hkv, dim=nh).float()).sum(-1)
        if tensor_layout == "NHD":
            lse_correction = lse_correction.transpose(1, 2)
    return _finish(o, lse, head_dim_og, return_lse, smooth_k, lse_correction, sm_scale)
