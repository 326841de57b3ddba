"""FP8-PV attention for Q / K rows of 129 .. 192 channels against V rows of up to 128 (gfx950): ``sageattn_qk192``.

Every other entry of the package wants ``k`` and ``v`` of one shape.  The multi-head-latent-attention prefill of the DeepSeek-V2 / V3 / R1
line has Q and K rows of 192 channels (128 "nope" + 64 rope) and V rows of 128; through ``sageattn_hd256`` it costs a V padded to the width of K
and everything padded to 256.  This module is the arithmetic of the default FP8 route -- K smoothed by its per-channel mean, per-thread INT8 Q
and K, the exact score form, e4m3 V with a per-channel scale at ``scale_max = 448``, two-level FP32 accumulation -- on kernels written for
192 / 128 (include/sage_qk192_gfx950.h).  The import path is ``sageattention_amd.qk192``; the package's ``__all__`` is the
reference's list and stays so.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import _cabi, _cabi_qk192
from .core import _finish
from .quant import _aligned, _dims, _p, _stream

HEAD_DIM_QK, HEAD_DIM_V = 192, 128


def _check(q, k, v, tensor_layout):
    if torch.compiler.is_compiling():
        raise ValueError("sageattn_qk192 is not supported under torch.compile: call it from eager code (torch.compiler.disable)")
    if tensor_layout not in ("HND", "NHD"):
        raise ValueError(f"Unknown tensor layout: {tensor_layout}")
    if not (q.dim() == k.dim() == v.dim() == 4):
        raise ValueError(f"q, k, v must be 4-D (got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})")
    dqk, dv = q.size(-1), v.size(-1)
    if dqk <= 128:
        raise ValueError(f"sageattn_qk192 takes 128 < head_dim of q and k <= 192 (got {dqk}): call sageattention_amd.sageattn for head_dim <= 128")
    if dqk > 256:
        raise ValueError(f"Unsupported head_dim: {dqk} (sageattn_qk192 takes 128 < head_dim of q and k <= 192; split the heads, or call "
                         "torch.nn.functional.scaled_dot_product_attention)")
    if dqk > HEAD_DIM_QK or dv > HEAD_DIM_V:
        raise ValueError(f"sageattn_qk192 takes 128 < head_dim of q and k <= 192 and head_dim of v <= 128 (got {dqk} and {dv}): call "
                         "sageattention_amd.hd256.sageattn_hd256 with v zero-padded to the head_dim of k, and slice its output")
    if dv < 1:
        raise ValueError("head_dim of v must be at least 1")
    if not (q.is_cuda and k.is_cuda and v.is_cuda and q.device == k.device == v.device):
        raise ValueError("sageattn_qk192 needs q, k and v on one CUDA (ROCm) device: move them with .cuda(); there is no CPU path")
    if q.dtype not in (torch.float16, torch.bfloat16) or not (q.dtype == k.dtype == v.dtype):
        raise ValueError(f"q, k, v must share one dtype, torch.float16 or torch.bfloat16 (got {q.dtype}, {k.dtype}, {v.dtype}): cast with .half() / .bfloat16()")
    qd, kd, vd = _dims(q, tensor_layout)[:4], _dims(k, tensor_layout)[:4], _dims(v, tensor_layout)[:4]
    if kd[:3] != vd[:3] or (qd[0], qd[3]) != (kd[0], kd[3]):
        raise ValueError(f"k and v must agree in batch, heads and length, and k with q in batch and head_dim (got q {tuple(q.shape)}, "
                         f"k {tuple(k.shape)}, v {tuple(v.shape)}, layout {tensor_layout})")
    if qd[1] % kd[1] != 0:
        raise ValueError(f"num_qo_heads ({qd[1]}) must be divisible by num_kv_heads ({kd[1]})")
    if qd[2] < 1 or kd[2] < 1:
        raise ValueError("qo_len and kv_len must be at least 1")
    if not (q.stride(-1) == k.stride(-1) == v.stride(-1) == 1):
        raise ValueError("Last dim of qkv must be contiguous: call .contiguous()")


def sageattn_qk192(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tensor_layout: str = "HND", is_causal: bool = False,
                   sm_scale: Optional[float] = None, smooth_k: bool = True, return_lse: bool = False):
    """INT8 QK^T + FP8 (e4m3) PV attention for ``q`` and ``k`` of ``128 < Dqk <= 192`` channels (zero-padded to 192) and ``v`` of
    ``1 <= Dv <= 128`` (zero-padded to 128); the output is ``[..., Dv]`` in the layout and dtype given.  fp16 / bf16 inputs in "HND" or "NHD"
    layout, GQA (``Hq % Hkv == 0``), any ``qo_len >= 1`` and ``kv_len >= 1``, top-left causal.  ``sm_scale`` defaults to ``Dqk ** -0.5``.
    ``return_lse`` as for ``sageattn_qk_int8_pv_fp8_cuda``: ``(o, lse)`` with the natural-log LSE ``[B, Hq, qo_len]``.  Everything else
    raises ``ValueError`` and names the entry to call: ``Dqk <= 128`` (``sageattn``), ``Dqk > 192`` or ``Dv > 128`` (``sageattn_hd256`` with
    ``v`` padded), a wrong dtype or device, mismatched shapes, use under torch.compile."""
    _check(q, k, v, tensor_layout)
    torch.cuda.set_device(q.device)
    dqk_og, dv_og = q.size(-1), v.size(-1)
    if sm_scale is None:
        sm_scale = dqk_og ** -0.5
    if dqk_og < HEAD_DIM_QK:
        q, k = F.pad(q, (0, HEAD_DIM_QK - dqk_og)), F.pad(k, (0, HEAD_DIM_QK - dqk_og))
    if dv_og < HEAD_DIM_V:
        v = F.pad(v, (0, HEAD_DIM_V - dv_og))
    q, k, v = _aligned(q, 8), _aligned(k, 8), _aligned(v, 8)
    lib = _cabi_qk192.load()
    B, Hq, Lq, DQK, q_sb, q_sh, q_sl = _dims(q, tensor_layout)
    _, Hkv, Lk, _, k_sb, k_sh, k_sl = _dims(k, tensor_layout)
    _, _, _, DV, v_sb, v_sh, v_sl = _dims(v, tensor_layout)
    dev = q.device
    ntile = (Lk + 63) // 64
    code = _cabi.DTYPE_F16 if q.dtype == torch.float16 else _cabi.DTYPE_BF16
    k_img = torch.empty((B, Hkv, ntile, 64 * DQK), dtype=torch.uint8, device=dev)
    v_img = torch.empty((B, Hkv, ntile, 64 * DV), dtype=torch.uint8, device=dev)
    k_scale = torch.empty((B, Hkv, 4 * ntile), dtype=torch.float32, device=dev)
    v_scale = torch.empty((B, Hkv, DV), dtype=torch.float32, device=dev)
    k_mean = torch.empty((B, Hkv, DQK), dtype=q.dtype, device=dev)
    ws_floats = lib.sage_qk192_ws_floats(B, Hkv, Lk)
    ws = torch.empty((ws_floats,), dtype=torch.float32, device=dev)
    rc = lib.sage_qk192_prepass(_p(k), _p(v), _p(k_img), _p(k_scale), _p(k_mean), _p(v_img), _p(v_scale), _p(ws), ws_floats, B, Hkv, Lk, DQK, DV,
                                k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, int(bool(smooth_k)), code, _stream(q))
    _cabi.check(rc, "sage_qk192_prepass")
    o = torch.empty(q.shape[:-1] + (DV,), dtype=q.dtype, device=dev)
    _, _, _, _, o_sb, o_sh, o_sl = _dims(o, tensor_layout)
    lse = torch.empty((B, Hq, Lq), dtype=torch.float32, device=dev) if return_lse else None
    rc = lib.sage_qk192_attn(_p(q), _p(k_img), _p(v_img), _p(k_scale), _p(v_scale), _p(o), _p(lse), B, Hq, Hkv, Lq, Lk, DQK, DV,
                             q_sb, q_sh, q_sl, o_sb, o_sh, o_sl, int(bool(is_causal)), float(sm_scale), code, _stream(q))
    _cabi.check(rc, "sage_qk192_attn")
    lse_correction = None
    if return_lse and smooth_k:
        km = k_mean.unsqueeze(1 if tensor_layout == "NHD" else 2)      # [B, 1, Hkv, D] / [B, Hkv, 1, D]: k.mean(dim=seq, keepdim=True)
        # q . km^T per row in FP32 (over 192 channels the product's rounding to bf16 would cost the LSE close to 1e-2), km broadcast over the GQA group
        nh = 2 if tensor_layout == "NHD" else 1
        lse_correction = (q.float() * torch.repeat_interleave(km, Hq // Hkv, dim=nh).float()).sum(-1)
        if tensor_layout == "NHD":
            lse_correction = lse_correction.transpose(1, 2)
    return _finish(o, lse, dv_og, return_lse, smooth_k, lse_correction, sm_scale)
