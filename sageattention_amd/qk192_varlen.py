"""Packed variable-length FP8-PV attention for Q / K rows of 129 .. 192 channels against V rows of up to 128 (gfx950): ``sageattn_qk192_varlen``.

``sageattn_qk192`` (:mod:`qk192`) is a dense call: one ``Lq`` and one ``Lk`` for the batch, top-left causal.  Serving stacks run the
multi-head-latent-attention prefill as FlashAttention's varlen call -- ``q [total_q, Hq, 192]``, ``k [total_k, Hkv, 192]``,
``v [total_k, Hkv, 128]`` behind ``cu_seqlens_q`` / ``cu_seqlens_k``, causal aligned bottom-right, a chunk of rows against an already cached
prefix.  This module is that call on the dense route's kernels (include/sage_qk192v_gfx950.h): every sequence is the dense call
on its own slice.  The import path is ``sageattention_amd.qk192_varlen``; the package's ``__all__`` is the reference's list and stays so.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import _cabi, _cabi_qk192v
from .core import _finish
from .qk192 import HEAD_DIM_QK, HEAD_DIM_V
from .quant import _aligned, _p, _stream

_MASKS = {(False, "top_left"): _cabi_qk192v.MASK_NONE, (False, "bottom_right"): None,
          (True, "top_left"): _cabi_qk192v.MASK_TOP_LEFT, (True, "bottom_right"): _cabi_qk192v.MASK_BOTTOM_RIGHT}
MAX_SEQS = 1024       # kVarlenPlanMaxSeq: the sequences one plan launch takes


def size_bounds(total_q: int, total_k: int, nseq: int):
    """(work items, 64-key tiles, 256-token statistics chunks) the call's buffers and grids are sized for on the host: a sequence rounds each
    count up by less than one, so the sums over any split of the rows into ``nseq`` sequences stay inside."""
    return (total_q + 127) // 128 + nseq, (total_k + 63) // 64 + nseq, (total_k + 255) // 256 + nseq


def _check(q, k, v, cu_seqlens_q, cu_seqlens_k, is_causal, causal_align):
    name = "sageattn_qk192_varlen"
    if torch.compiler.is_compiling():
        raise ValueError(f"{name} is not supported under torch.compile: call it from eager code (torch.compiler.disable)")
    if not isinstance(causal_align, str) or causal_align not in ("top_left", "bottom_right"):
        raise ValueError(f'causal_align must be "top_left" or "bottom_right" (got {causal_align!r})')
    if _MASKS[(bool(is_causal), causal_align)] is None:
        raise ValueError('causal_align="bottom_right" needs is_causal=True (a call without a causal mask takes causal_align="top_left")')
    if not (q.dim() == k.dim() == v.dim() == 3):
        raise ValueError(f"q, k, v must be packed 3-D [tokens, heads, head_dim] (got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}): "
                         "call sageattention_amd.qk192.sageattn_qk192 for a dense [B, H, L, D] batch")
    dqk, dv = q.size(-1), v.size(-1)
    if dqk <= 128:
        raise ValueError(f"{name} takes 128 < head_dim of q and k <= 192 (got {dqk}): call sageattention_amd.sageattn_qk_int8_pv_fp8_varlen "
                         "for head_dim <= 128")
    if dqk > HEAD_DIM_QK or dv > HEAD_DIM_V:
        raise ValueError(f"{name} takes 128 < head_dim of q and k <= 192 and head_dim of v <= 128 (got {dqk} and {dv}): no packed route is wider; "
                         "call sageattention_amd.hd256.sageattn_hd256 per sequence with v zero-padded to the head_dim of k, and slice its output")
    if dv < 1:
        raise ValueError("head_dim of v must be at least 1")
    if not (q.is_cuda and k.is_cuda and v.is_cuda and q.device == k.device == v.device):
        raise ValueError(f"{name} needs q, k and v on one CUDA (ROCm) device: move them with .cuda(); there is no CPU path")
    if q.dtype not in (torch.float16, torch.bfloat16) or not (q.dtype == k.dtype == v.dtype):
        raise ValueError(f"q, k, v must share one dtype, torch.float16 or torch.bfloat16 (got {q.dtype}, {k.dtype}, {v.dtype}): cast with .half() / .bfloat16()")
    if k.shape[:2] != v.shape[:2] or k.size(-1) != dqk:
        raise ValueError(f"k and v must agree in tokens and heads, and k with q in head_dim (got q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)})")
    if q.size(1) % k.size(1) != 0:
        raise ValueError(f"num_qo_heads ({q.size(1)}) must be divisible by num_kv_heads ({k.size(1)})")
    if not (q.stride(-1) == k.stride(-1) == v.stride(-1) == 1):
        raise ValueError("Last dim of qkv must be contiguous: call .contiguous()")
    for what, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if not isinstance(cu, torch.Tensor) or cu.dtype != torch.int32 or cu.dim() != 1 or cu.device != q.device:
            raise ValueError(f"{what} must be a 1-D torch.int32 tensor on the device of q: cast with .to(torch.int32) and move it with .cuda()")
    if cu_seqlens_q.numel() != cu_seqlens_k.numel() or not 2 <= cu_seqlens_q.numel() <= MAX_SEQS + 1:
        raise ValueError(f"cu_seqlens_q and cu_seqlens_k must both hold nseq + 1 entries, 1 <= nseq <= {MAX_SEQS} (got {cu_seqlens_q.numel()} and "
                         f"{cu_seqlens_k.numel()}): split a longer batch into calls of at most {MAX_SEQS} sequences")


def sageattn_qk192_varlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor, cu_seqlens_k: torch.Tensor,
                          max_seqlen_q: int, max_seqlen_k: int, is_causal: bool = False, causal_align: str = "bottom_right",
                          sm_scale: Optional[float] = None, smooth_k: bool = True, return_lse: bool = False):
    """INT8 QK^T + FP8 (e4m3) PV attention over a packed batch: ``q [total_q, Hq, Dqk]``, ``k [total_k, Hkv, Dqk]`` with ``128 < Dqk <= 192``
    (zero-padded to 192), ``v [total_k, Hkv, Dv]`` with ``1 <= Dv <= 128`` (zero-padded to 128), fp16 / bf16, GQA (``Hq % Hkv == 0``);
    ``cu_seqlens_q`` / ``cu_seqlens_k`` int32 ``[nseq + 1]`` on the device, ``nseq <= 1024``.  Returns ``o [total_q, Hq, Dv]`` and, with
    ``return_lse``, the natural-log LSE ``[Hq, total_q]`` in fp32 (the layout of ``sageattn_qk_int8_pv_fp8_varlen``).  ``sm_scale`` defaults to
    ``Dqk ** -0.5``.

    Every sequence is ``sageattn_qk192`` on its own slice: the K mean is per (sequence, kv head) over that sequence's keys, the INT8 K scale
    groups sit on 64-key tiles and the Q groups on 128-row blocks counted from the sequence's first key / row, the V scale is per (sequence, kv
    head, channel).  Without a mask and with ``causal_align="top_left"`` the rows of a sequence are bit for bit the dense call's on that slice.
    ``causal_align="bottom_right"`` (the default of the keyword; it needs ``is_causal=True``): row i of sequence s sees key j iff
    ``j <= i + Lk_s - Lq_s`` -- a chunk of rows against a cached prefix.  Rows in front of key 0, and every row of a sequence without keys, give
    ``o = +0`` and ``lse = -inf``; a sequence without rows contributes nothing.

    No host synchronisation, graph capturable: buffers and grids are sized from ``total_q``, ``total_k`` and ``nseq`` (``size_bounds``), the true
    counts stay on the device.  ``max_seqlen_q`` / ``max_seqlen_k`` are FlashAttention's arguments and size nothing here.  Everything else raises
    ``ValueError`` and names the entry to call: ``Dqk <= 128`` (``sageattn_qk_int8_pv_fp8_varlen``), ``Dqk > 192`` or ``Dv > 128``, a wrong dtype
    or device, ``cu_seqlens`` of the wrong dtype or length, ``bottom_right`` without ``is_causal``, use under torch.compile."""
    _check(q, k, v, cu_seqlens_q, cu_seqlens_k, is_causal, causal_align)
    torch.cuda.set_device(q.device)
    mask = _MASKS[(bool(is_causal), causal_align)]
    dqk_og, dv_og = q.size(-1), v.size(-1)
    if sm_scale is None:
        sm_scale = dqk_og ** -0.5
    total_q, Hq = q.shape[:2]
    total_k, Hkv = k.shape[:2]
    nseq = cu_seqlens_q.numel() - 1
    dev = q.device
    if total_q == 0 or total_k == 0:       # (shapes, not lengths: nothing to launch; without a key every row is in front of key 0)
        o = torch.zeros((total_q, Hq, dv_og), dtype=q.dtype, device=dev)
        return (o, torch.full((Hq, total_q), float("-inf"), dtype=torch.float32, device=dev)) if return_lse else o
    if dqk_og < HEAD_DIM_QK:
        q, k = F.pad(q, (0, HEAD_DIM_QK - dqk_og)), F.pad(k, (0, HEAD_DIM_QK - dqk_og))
    if dv_og < HEAD_DIM_V:
        v = F.pad(v, (0, HEAD_DIM_V - dv_og))
    q, k, v = _aligned(q, 8), _aligned(k, 8), _aligned(v, 8)
    cu_q, cu_k = cu_seqlens_q.contiguous(), cu_seqlens_k.contiguous()
    lib = _cabi_qk192v.load()
    _, tiles, _ = size_bounds(total_q, total_k, nseq)
    code = _cabi.DTYPE_F16 if q.dtype == torch.float16 else _cabi.DTYPE_BF16
    k_img = torch.empty((Hkv, tiles, 64 * HEAD_DIM_QK), dtype=torch.uint8, device=dev)
    v_img = torch.empty((Hkv, tiles, 64 * HEAD_DIM_V), dtype=torch.uint8, device=dev)
    k_scale = torch.empty((Hkv, 4 * tiles), dtype=torch.float32, device=dev)
    v_scale = torch.empty((nseq, Hkv, HEAD_DIM_V), dtype=torch.float32, device=dev)
    k_mean = torch.empty((nseq, Hkv, HEAD_DIM_QK), dtype=q.dtype, device=dev)
    ws_bytes = lib.sage_qk192v_ws_bytes(nseq, Hkv, total_q, total_k)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    rc = lib.sage_qk192v_prepass(_p(k), _p(v), _p(cu_q), _p(cu_k), _p(k_img), _p(k_scale), _p(k_mean), _p(v_img), _p(v_scale), _p(ws), ws_bytes,
                                 nseq, total_q, total_k, Hq, Hkv, HEAD_DIM_QK, HEAD_DIM_V, k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                                 mask, int(bool(smooth_k)), code, _stream(q))
    _cabi.check(rc, "sage_qk192v_prepass")
    o = torch.empty((total_q, Hq, HEAD_DIM_V), dtype=q.dtype, device=dev)
    lse = torch.empty((Hq, total_q), dtype=torch.float32, device=dev) if return_lse else None
    rc = lib.sage_qk192v_attn(_p(q), _p(cu_q), _p(cu_k), _p(k_img), _p(v_img), _p(k_scale), _p(v_scale), _p(ws), ws_bytes, _p(o), _p(lse),
                              nseq, total_q, total_k, Hq, Hkv, HEAD_DIM_QK, HEAD_DIM_V, q.stride(0), q.stride(1), o.stride(0), o.stride(1),
                              mask, float(sm_scale), code, _stream(q))
    _cabi.check(rc, "sage_qk192v_attn")
    lse_correction = None
    if return_lse and smooth_k:
        # q . mean of the row's OWN sequence, per row in FP32 over the 192 channels as the dense call forms it; row -> sequence on the device
        # (the number of prefix entries <= row, the rows behind the last prefix with the last sequence)
        seq_of_row = torch.bucketize(torch.arange(total_q, dtype=torch.int32, device=dev), cu_q[1:], right=True).clamp_(max=nseq - 1)
        km = torch.repeat_interleave(k_mean.index_select(0, seq_of_row), Hq // Hkv, dim=1)            # [total_q, Hq, 192]
        lse_correction = (q.float() * km.float()).sum(-1).transpose(0, 1)
    return _finish(o, lse, dv_og, return_lse, smooth_k, lse_correction, sm_scale)
