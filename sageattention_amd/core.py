"""Public API of sageattention_amd -- the drop-in for ``sageattention/core.py`` on MI355X.

Same six public names, same signatures, same kwargs and error behaviour as the reference
(``/root/reference/sageattention/core.py``: ``sageattn`` :79, ``sageattn_qk_int8_pv_fp16_triton``
:160, ``sageattn_varlen`` :334, ``sageattn_qk_int8_pv_fp16_cuda`` :451,
``sageattn_qk_int8_pv_fp8_cuda`` :636, ``sageattn_qk_int8_pv_fp8_cuda_sm90`` :829), so
``F.scaled_dot_product_attention = sageattn`` in the CogVideoX / Hunyuan / Wan examples keeps
working.  Host code here is plumbing only (padding, K mean, allocation, LSE fix-up -- exactly
what the reference does in Python); every tensor-sized computation, including the K-smoothing
mean, runs in the hand-written HIP kernels behind ``libsage_gfx950.so``.  There is no fallback path: CPU
tensors or a missing library raise.
"""
from __future__ import annotations

import os

import ctypes
import warnings
from typing import Any, NamedTuple, Optional

import torch
import torch.nn.functional as F

from . import _cabi, _cabi_kvpaged, _cabi_kvpsplit, ops
from .quant import (LOG2E, _aligned, _cu_blocks, _dims, _p, _quant, _squeeze_km, _stream, channel_mean, channel_mean_kvlens, channel_mean_packed,
                    per_block_int8, per_block_int8_varlen, per_channel_fp8, per_channel_fp8_kvlens, per_channel_fp8_varlen, per_thread_int8_k_kvlens, prep_v_fp16, prep_v_fp16_varlen, prepass_fused_ok, prepass_kv_fp8, prepass_kv_varlen,
                    prepass_varlen_fused_ok, sub_mean, varlen_plan)

_SUPPORTED_ARCH_PREFIX = "gfx950"
_FUSE_Q16_DEFAULT = os.environ.get("SAGE_FUSE_Q16", "1") != "0"      # debugging switch


def get_gcn_arch(device: torch.device) -> str:
    """ROCm analogue of the reference's ``get_cuda_arch_versions`` (core.py:71-76)."""
    return torch.cuda.get_device_properties(device).gcnArchName.split(":")[0]


def _check_shapes(q, k, v, tensor_layout: Optional[str] = "HND", cu_seqlens_q=None, cu_seqlens_k=None):
    """Refuse operands that do not agree, before any launch: the C ABI takes raw pointers and one set of sizes, so a ``v`` with fewer tokens
    or heads than ``k`` would be read past its end (the reference refuses at its op boundary, ``CHECK_SHAPE(value, ...)``,
    qk_int_sv_f16_cuda_sm80.cu:731-751).  Dense (``tensor_layout`` "HND" / "NHD"): k and v agree in batch, kv-head count, length and head
    dim, q and k in batch and head dim.  Packed (``tensor_layout=None``, ``[sum L, H, D]``): k and v have one shape, q and k one head dim,
    the two prefix arrays one length.  That ``cu_seqlens_*[-1]`` stays within the packed rows is NOT checked: it would take a device-to-host
    read on every call and break graph capture."""
    if tensor_layout is None:
        assert q.dim() == 3 and k.dim() == 3 and v.dim() == 3, f"packed q, k, v must be [sum L, H, D] (got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})"
        assert k.shape == v.shape, f"k and v must have the same shape (got k {tuple(k.shape)}, v {tuple(v.shape)})"
        assert q.shape[2] == k.shape[2], f"q and k must have the same head_dim (got q {tuple(q.shape)}, k {tuple(k.shape)})"
        assert cu_seqlens_q.dim() == 1 and cu_seqlens_q.shape == cu_seqlens_k.shape, \
            f"cu_seqlens_q and cu_seqlens_k must be 1-D and of one length (got {tuple(cu_seqlens_q.shape)}, {tuple(cu_seqlens_k.shape)})"
        return
    assert q.dim() == 4 and k.dim() == 4 and v.dim() == 4, f"q, k, v must be 4-D (got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})"
    qB, _, _, qD = _dims(q, tensor_layout)[:4]
    kB, kH, kL, kD = _dims(k, tensor_layout)[:4]
    assert (kB, kH, kL, kD) == _dims(v, tensor_layout)[:4], \
        f"k and v must agree in batch, kv-head count, length and head_dim (got k {tuple(k.shape)}, v {tuple(v.shape)}, layout {tensor_layout})"
    assert (qB, qD) == (kB, kD), f"q and k must agree in batch and head_dim (got q {tuple(q.shape)}, k {tuple(k.shape)}, layout {tensor_layout})"


def _check_inputs(q, k, v):
    dtype = q.dtype
    assert q.is_cuda, "Input tensors must be on cuda."
    assert dtype in [torch.float16, torch.bfloat16], "Input tensors must be in dtype of torch.float16 or torch.bfloat16"
    assert q.device == k.device == v.device, "All tensors must be on the same device."
    assert q.dtype == k.dtype == v.dtype, "All tensors must have the same dtype."


def _pad_head_dim(q, k, v):
    """core.py:260-271: zero-pad head_dim to 64 / 128; > 128 is rejected."""
    head_dim_og = q.size(-1)
    if head_dim_og < 64:
        q, k, v = (F.pad(t, (0, 64 - head_dim_og)) for t in (q, k, v))
    elif 64 < head_dim_og < 128:
        q, k, v = (F.pad(t, (0, 128 - head_dim_og)) for t in (q, k, v))
    elif head_dim_og > 128:
        raise ValueError(f"Unsupported head_dim: {head_dim_og}")
    return q, k, v, head_dim_og


def _lse_correction(q, km, tensor_layout):
    """core.py:283-293: q . km^T per query row (fp32), km broadcast over the GQA group."""
    nh_dim = 2 if tensor_layout == "NHD" else 1
    g = q.size(nh_dim) // km.size(nh_dim)
    km_b = torch.repeat_interleave(km, g, dim=nh_dim) if g > 1 else km
    if tensor_layout == "NHD":
        return torch.matmul(q.transpose(1, 2), km_b.transpose(1, 2).transpose(2, 3)).squeeze(-1).to(torch.float32)
    return torch.matmul(q, km_b.transpose(2, 3)).squeeze(-1).to(torch.float32)


def _smooth_k(q, k, tensor_layout, smooth_k, return_lse):
    """core.py:279-295: km = mean of k over the sequence (keepdim), and q.km^T for the LSE fix-up."""
    if not smooth_k:
        return None, None
    seq_dim = 1 if tensor_layout == "NHD" else 2
    km = channel_mean(k, tensor_layout).unsqueeze(seq_dim)     # k.mean(dim=seq_dim, keepdim=True) as a HIP reduction
    return km, (_lse_correction(q, km, tensor_layout) if return_lse else None)


def _attn_dense(fp8, q_int8, k_int8, v_image, v_scale, q_scale, k_scale, out_dtype, tensor_layout, is_causal,
                gran, q_warp, sm_scale_log2, two_level, return_lse, v_mean=None, folded_scores=False):
    """Allocate ``o`` and launch the fused kernel through the registered custom op (-> C ABI)."""
    B, Hq, Lq, D, _, _, _ = _dims(q_int8, tensor_layout)
    Hkv = _dims(k_int8, tensor_layout)[1]
    assert Hq % Hkv == 0, "num_qo_heads must be divisible by num_kv_heads"
    o = torch.empty(q_int8.shape, dtype=out_dtype, device=q_int8.device)
    layout = 0 if tensor_layout == "NHD" else 1            # the reference's encoding (core.py:556)
    # two_level: True / False, or "triton" = the Triton kernel form of the FP16-PV entry point (_cabi.PV_ACCUM_TRITON)
    accum = _cabi.PV_ACCUM_TRITON if two_level == "triton" else (_cabi.PV_ACCUM_TWO_LEVEL if two_level else _cabi.PV_ACCUM_SINGLE)
    # Under torch.compile the registered custom ops are traced; in eager mode their implementations are
    # called directly (same code, minus ~15 us of dispatcher overhead per call).
    compiling = torch.compiler.is_compiling()
    f8 = ops.qk_int8_sv_f8_attn if compiling else ops.qk_int8_sv_f8_attn_impl
    f16 = ops.qk_int8_sv_f16_attn if compiling else ops.qk_int8_sv_f16_attn_impl
    if fp8:
        lse = f8(q_int8, k_int8, v_image, o, q_scale, k_scale, v_scale, v_mean, layout, int(is_causal),
                 gran, q_warp, float(sm_scale_log2), accum, int(return_lse), bool(folded_scores))
    else:
        lse = f16(q_int8, k_int8, v_image, o, q_scale, k_scale, v_mean, layout, int(is_causal),
                  gran, q_warp, float(sm_scale_log2), accum, int(return_lse))
    return o, (lse if return_lse else None)


def _v_rows_ok(v, tensor_layout: str) -> bool:
    """Whether an fp16 V tensor can be read in place by the FP16-PV kernels (``sage_attn_fused_q*_pv_f16_vrows``): 16-byte rows."""
    if v.dtype != torch.float16 or v.stride(-1) != 1 or v.data_ptr() % 16 != 0:
        return False
    _, _, L, D, sb, sh, sl = _dims(v, tensor_layout)
    return sb % 8 == 0 and sh % 8 == 0 and sl % 8 == 0 and sl >= D and ((L - 1) * sl + D) * 2 < 2 ** 31


_V_IN_PLACE = {"0": False, "1": True}.get(os.environ.get("SAGE_V_IN_PLACE", ""))      # 0 / 1: force the route for every eligible call (A/B, debugging)


def _v_rows_wanted(q, k, v, tensor_layout: str, is_causal: bool, override) -> bool:
    """Whether an FP16-PV call on fp16 inputs reads V's rows in place instead of building the tile image.  Same bits either way.  Measured
    (profiles/r6_run_e_vrows_ab.txt, B2 H32 D128): the K-only pre-pass is 24-100 us shorter than K + V image (46 vs 72 us at N = 4096, 116 vs
    214 at 16384: 4 of its 7 bytes per element gone), the attention kernel 2.2-3.7 % slower (twice the LDS read instructions for the V operand:
    64-bit transposing reads); whole call + 6.5 % at C2 (N = 4096 causal), + 7-8 % at N = 2048, + 1.6-3 % at N = 4096 non-causal, 0 at N = 16384
    causal.  The saving grows with Lk per kv-head, the loss with the (query, key) pairs per query head: rows in place up to
    (Hq / Hkv) * Lq * (1/2 if causal) = 6144, the image beyond."""
    if not _v_rows_ok(v, tensor_layout):
        return False
    if override is None:
        override = _V_IN_PLACE
    if override is not None:
        return bool(override)
    _, Hq, Lq = _dims(q, tensor_layout)[:3]
    Hkv = _dims(k, tensor_layout)[1]
    return (Hq // Hkv) * Lq * (0.5 if is_causal else 1.0) <= 6144


@torch.compiler.disable
def _attn_fused_q(q, k_int8, v_image, v_scale, k_scale, tensor_layout, is_causal, sm_scale_log2, return_lse, v_mean=None, folded_scores=False,
                  v_rows=False, kv_lens=None, q_start=None, window=0, gqa_pack=False, num_splits=0, paged=None):
    """FP8-PV two-level attention with the per-thread Q quantisation done in the kernel prologue
    (``sage_attn_fused_q_pv_f8``): bit-identical to ``per_thread_int8`` + the attention op, one launch and
    3 B/element of HBM traffic less.  ``v_rows`` (FP16 PV): ``v_image`` is the fp16 V tensor itself, read in place.
    ``kv_lens`` (FP8 PV, int32 [B] on the device): a key length per sample (``sage_attn_fused_q_pv_f8_kvlens``); ``q_start`` (with
    ``kv_lens``, causal; int32 [B] on the device): a query offset per sample (``SageLaunchAttr.q_start``); ``window`` (with ``kv_lens``,
    causal; a Python int): the number of keys a row sees up to and including its diagonal, 0 = unbounded (``SageLaunchAttr.window``);
    ``gqa_pack`` (with ``kv_lens``, ``Lq <= 32``, ``Hq / Hkv >= 2``): the query heads of a GQA group four to a workgroup (``SAGE_ATTR_GQA_PACK``);
    ``num_splits`` (with ``kv_lens``, ``Lq <= 128``, no window; 0 or 2 .. 255): that many key-range chunks, exactly (``SAGE_ATTR_KV_SPLIT``; the
    split workspace is allocated here, from the shapes alone); ``paged`` (with ``kv_lens``; a ``PagedQuantizedKVCache``): ``k_int8`` /
    ``v_image`` / ``k_scale`` are its pool of pages and the call goes through its block table (``sage_kvpaged_attn``), which takes the offsets,
    the window and the packing flag and nothing else of the attributes -- or, with ``num_splits``, ``sage_kvpsplit_attn``, the exact split
    on the pool, which takes the offsets, the packing flag, the chunk count and the split workspace."""
    B, Hq, Lq, D, q_sb, q_sh, q_sl = _dims(q, tensor_layout)
    _, Hkv, Lk, _, k_sb, k_sh, k_sl = _dims(k_int8, tensor_layout)
    assert Hq % Hkv == 0, "num_qo_heads must be divisible by num_kv_heads"
    o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    _, _, _, _, o_sb, o_sh, o_sl = _dims(o, tensor_layout)
    lse = torch.empty((B, Hq, Lq), dtype=torch.float32, device=q.device) if return_lse else None
    code = _cabi.DTYPE_F16 if q.dtype == torch.float16 else _cabi.DTYPE_BF16
    # (a large non-causal call: persistent launch; FP8 PV: the score form)
    assert (q_start is None and not window) or (kv_lens is not None and is_causal)
    assert not gqa_pack or kv_lens is not None
    assert not num_splits or (kv_lens is not None and not window and Lq <= 128)
    split_ws = torch.empty((_cabi.kv_split_ws_bytes(B, Hq, Lq, D, num_splits) // 4,), dtype=torch.float32, device=q.device) if num_splits else None
    if paged is not None:          # (no launch workspace, no trace buffer, no forced ticket route: the C entry's ordinary dispatch)
        assert kv_lens is not None
        attr = _cabi.launch_attr(launch_ws=split_ws, grid_out=ops._hooks.grid_probe, q_start=q_start, window=window, gqa_pack=gqa_pack, kv_split=num_splits)
    else:
        attr = ops.attn_attr(q.device, is_causal, B * Hq * ((Lq + 127) // 128), folded_scores and v_scale is not None, q_start=q_start, window=window,
                             gqa_pack=gqa_pack, kv_split=num_splits, split_ws=split_ws)
    if v_rows:                     # FP16 PV on fp16 inputs: V rows in place, no tile image (sage_attn_fused_q_pv_f16_vrows)
        assert v_scale is None and v_mean is None
        _, _, _, _, v_sb, v_sh, v_sl = _dims(v_image, tensor_layout)
        rc = _cabi.load().sage_attn_fused_q_pv_f16_vrows(
            _p(q), _p(k_int8), _p(v_image), _p(o), _p(lse), _p(k_scale),
            B, Hq, Hkv, Lq, Lk, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, o_sb, o_sh, o_sl,
            int(is_causal), float(sm_scale_log2), code, _stream(q), _cabi.attr_arg(attr))
        ops.attn_check(rc, "sage_attn_fused_q_pv_f16_vrows", attr, q.device)
        return o, lse
    if v_scale is None:            # FP16 PV (v_image from prep_v_fp16), straight FP32 accumulation
        rc = _cabi.load().sage_attn_fused_q_pv_f16(
            _p(q), _p(k_int8), _p(v_image), _p(o), _p(lse), _p(k_scale), _p(v_mean),
            B, Hq, Hkv, Lq, Lk, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, o_sb, o_sh, o_sl,
            int(is_causal), float(sm_scale_log2), code, code, _stream(q), _cabi.attr_arg(attr))
        ops.attn_check(rc, "sage_attn_fused_q_pv_f16", attr, q.device)
        return o, lse
    if kv_lens is not None:
        assert v_scale is not None and not folded_scores and not v_rows
        if paged is not None and num_splits:      # the exact split on a pool of pages: the same three launches through the block table
            rc = _cabi_kvpsplit.load().sage_kvpsplit_attn(
                _p(q), _p(k_int8), _p(v_image), _p(o), _p(lse), _p(k_scale), _p(v_scale), _p(kv_lens),
                _p(paged.block_table), paged.block_table.stride(0), paged.num_pages, paged.page_size, paged.max_pages_per_seq,
                B, Hq, Hkv, Lq, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, o_sb, o_sh, o_sl,
                int(is_causal), float(sm_scale_log2), code, code, _stream(q), _cabi.attr_arg(attr))
            ops.attn_check(rc, "sage_kvpsplit_attn", attr, q.device)
            return o, lse
        if paged is not None:      # the same call on a pool of pages: Lk is the logical capacity, the K strides are a page's
            rc = _cabi_kvpaged.load().sage_kvpaged_attn(
                _p(q), _p(k_int8), _p(v_image), _p(o), _p(lse), _p(k_scale), _p(v_scale), _p(kv_lens),
                _p(paged.block_table), paged.block_table.stride(0), paged.num_pages, paged.page_size, paged.max_pages_per_seq,
                B, Hq, Hkv, Lq, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, o_sb, o_sh, o_sl,
                int(is_causal), float(sm_scale_log2), code, code, _stream(q), _cabi.attr_arg(attr))
            ops.attn_check(rc, "sage_kvpaged_attn", attr, q.device)
            return o, lse
        rc = _cabi.load().sage_attn_fused_q_pv_f8_kvlens(
            _p(q), _p(k_int8), _p(v_image), _p(o), _p(lse), _p(k_scale), _p(v_scale), _p(v_mean), _p(kv_lens),
            B, Hq, Hkv, Lq, Lk, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, o_sb, o_sh, o_sl,
            int(is_causal), float(sm_scale_log2), code, code, _stream(q), _cabi.attr_arg(attr))
        ops.attn_check(rc, "sage_attn_fused_q_pv_f8_kvlens", attr, q.device)
        return o, lse
    rc = _cabi.load().sage_attn_fused_q_pv_f8(
        _p(q), _p(k_int8), _p(v_image), _p(o), _p(lse), _p(k_scale), _p(v_scale), _p(v_mean),
        B, Hq, Hkv, Lq, Lk, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, o_sb, o_sh, o_sl,
        int(is_causal), float(sm_scale_log2), code, code, _stream(q), _cabi.attr_arg(attr))
    ops.attn_check(rc, "sage_attn_fused_q_pv_f8", attr, q.device)
    return o, lse


@torch.compiler.disable
def _attn_fused_qblock(q, k_int8, v_image, k_scale, tensor_layout, is_causal, q_premul, return_lse, v_rows=False):
    """The Triton-named API's attention with the per-block Q quantisation in the kernel prologue
    (``sage_attn_fused_qblock_pv_f16``): bit-identical to ``per_block_int8`` (q half) + the attention op.  ``v_rows``: ``v_image`` is the
    fp16 V tensor itself, read in place (``sage_attn_fused_qblock_pv_f16_vrows``)."""
    q = _aligned(q, 8)
    B, Hq, Lq, D, q_sb, q_sh, q_sl = _dims(q, tensor_layout)
    _, Hkv, Lk, _, k_sb, k_sh, k_sl = _dims(k_int8, tensor_layout)
    assert Hq % Hkv == 0, "num_qo_heads must be divisible by num_kv_heads"
    o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    _, _, _, _, o_sb, o_sh, o_sl = _dims(o, tensor_layout)
    lse = torch.empty((B, Hq, Lq), dtype=torch.float32, device=q.device) if return_lse else None
    code = _cabi.DTYPE_F16 if q.dtype == torch.float16 else _cabi.DTYPE_BF16
    attr = ops.attn_attr(q.device, is_causal, B * Hq * ((Lq + 127) // 128))
    if v_rows:
        _, _, _, _, v_sb, v_sh, v_sl = _dims(v_image, tensor_layout)
        rc = _cabi.load().sage_attn_fused_qblock_pv_f16_vrows(
            _p(q), _p(k_int8), _p(v_image), _p(o), _p(lse), _p(k_scale),
            B, Hq, Hkv, Lq, Lk, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, v_sb, v_sh, v_sl, o_sb, o_sh, o_sl,
            int(is_causal), float(q_premul), code, _stream(q), _cabi.attr_arg(attr))
        ops.attn_check(rc, "sage_attn_fused_qblock_pv_f16_vrows", attr, q.device)
        return o, lse
    rc = _cabi.load().sage_attn_fused_qblock_pv_f16(
        _p(q), _p(k_int8), _p(v_image), _p(o), _p(lse), _p(k_scale),
        B, Hq, Hkv, Lq, Lk, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, o_sb, o_sh, o_sl,
        int(is_causal), float(q_premul), code, code, _stream(q), _cabi.attr_arg(attr))
    ops.attn_check(rc, "sage_attn_fused_qblock_pv_f16", attr, q.device)
    return o, lse


def _split_kv_plan(B: int, Hq: int, Lq: int, Lk: int, is_causal: bool, override, auto_default: bool = True) -> int:
    """Number of key-range chunks S for a call whose grid would not fill the chip (0 = no split).  The reference kernels
    parallelise over (batch, head, 128-row q block) only, so few query rows against a long key range (cross-attention,
    decode-like shapes) leave most of the 256 CUs idle.  Such a call runs as
    S chunks of Lk/S keys folded into the kv-head dimension and one merge by log-sum-exp.  Chunks are whole numbers of
    64-key tiles (the quantisation groups and the V image tiles are unchanged by the fold), so only S | Lk/64 is considered.
    ``override``: 0 = never, an integer S >= 2 = that split, "auto" = the plan below, None = ``auto_default``.  The FP16-PV entry point
    plans by default (a split result meets the UNSPLIT oracle at the kernel tolerance: P is rounded to fp16).  The FP8-PV entry points do
    NOT (round 5): this split changes which running maximum every P is rounded to e4m3 against -- measured rel-RMS up to 2.8e-2 against the
    unsplit oracle, beyond the 1e-2 that a schedule variant may differ from the exact schedule by and still be a DEFAULT FP8 route
     -- so there it is opt-in (``split_kv="auto"`` or S), held to 2e-3 against the schedule-matched oracle as before.  The
    FP8 entry point's exact split (``split_kv_exact=True``, :func:`_split_exact_plan`) seeds every chunk with the unsplit call's running
    maximum instead: same P, only the FP32 summation order differs."""
    if override is None:
        override = "auto" if auto_default else 0
    if override == 0:
        return 0
    if override != "auto":
        if isinstance(override, bool) or not isinstance(override, int):
            raise ValueError(f"split_kv={override!r}: 0, an integer >= 2 or 'auto'")
        if Lk % 64 != 0 or override < 2 or (Lk // 64) % override != 0:
            raise ValueError(f"split_kv={override} must be >= 2 and divide the number of whole 64-key tiles (kv_len {Lk})")
        return override
    if Lk % 64 != 0:
        return 0
    ntk = Lk // 64
    n_wg = B * Hq * ((Lq + 127) // 128)
    if is_causal:
        # Causal calls are split only on request (split_kv=S; the mask then runs in global key coordinates).  Measured for the
        # case it could help -- one partial wave of workgroups, B=1 H=8 N=8192: 179 us unsplit, 199 us with S=4 -- the partial
        # outputs' extra pass through HBM and the merge cost more than the better balance returns (profiles/r2_run_z_shape_probe.txt).
        return 0
    else:
        if n_wg > 128 or ntk < 64:                     # the grid already covers half the chip, or the key range is short
            return 0
        target = max(2, min(ntk // 32, -(-768 // n_wg)))   # chunks of >= 32 tiles, about three workgroups per CU
    S = max(d for d in range(1, target + 1) if ntk % d == 0)
    return S if S >= 2 else 0


@torch.compiler.disable
def _attn_fused_q_split(q, k_int8, v_image, v_scale, k_scale, tensor_layout, is_causal, sm_scale_log2, S, return_lse, v_mean=None,
                        folded_scores=False):
    """Split-KV route of the fused-Q FP8 attention: the key range in S chunks folded into the kv-head dimension (zero-copy
    views of the INT8 K, its scales and the V image; Q is read in place by every chunk), partial outputs in fp16 +
    log2-domain log-sum-exps, one ``sage_merge_split`` pass."""
    B, Hq, Lq, D, q_sb, q_sh, q_sl = _dims(q, tensor_layout)
    _, Hkv, Lk, _, _, _, _ = _dims(k_int8, tensor_layout)
    group, Lc = Hq // Hkv, Lk // S
    k_store = k_int8 if tensor_layout == "HND" else k_int8.permute(0, 2, 1, 3)      # head-major storage (quant._quant)
    assert k_store.is_contiguous() and v_image.is_contiguous() and k_scale.is_contiguous()
    k_f = k_store.view(B, Hkv * S, Lc, D)
    ks_f = k_scale.view(B, Hkv * S, -1)
    vs_f = None if v_scale is None else v_scale.repeat_interleave(S, dim=1)      # None: FP16 PV (fp16 V image)
    vm_f = None if v_mean is None else v_mean.repeat_interleave(S, dim=1)
    o_part = torch.empty((B, Hq * S, Lq, D), dtype=torch.float16, device=q.device)
    lse_part = torch.empty((B, Hq * S, Lq), dtype=torch.float32, device=q.device)
    _, _, _, _, k_sb, k_sh, k_sl = _dims(k_f, "HND")
    _, _, _, _, p_sb, p_sh, p_sl = _dims(o_part, "HND")
    code = _cabi.DTYPE_F16 if q.dtype == torch.float16 else _cabi.DTYPE_BF16
    lib = _cabi.load()
    if vs_f is None:
        rc = lib.sage_attn_fused_q_pv_f16_split(
            _p(q), _p(k_f), _p(v_image), _p(o_part), _p(lse_part), _p(ks_f), _p(vm_f),
            B, Hq, Hkv, S, Lq, Lc, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, p_sb, p_sh, p_sl,
            int(is_causal), float(sm_scale_log2), code, _cabi.DTYPE_F16, _stream(q), None)
        _cabi.check(rc, "sage_attn_fused_q_pv_f16_split")
    else:
        rc = lib.sage_attn_fused_q_pv_f8_split(
            _p(q), _p(k_f), _p(v_image), _p(o_part), _p(lse_part), _p(ks_f), _p(vs_f), _p(vm_f),
            B, Hq, Hkv, S, Lq, Lc, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, p_sb, p_sh, p_sl,
            int(is_causal), float(sm_scale_log2), code, _cabi.DTYPE_F16, _stream(q),
            _cabi.attr_arg(_cabi.launch_attr(folded_scores=bool(folded_scores))))
        _cabi.check(rc, "sage_attn_fused_q_pv_f8_split")
    o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    _, _, _, _, o_sb, o_sh, o_sl = _dims(o, tensor_layout)
    lse = torch.empty((B, Hq, Lq), dtype=torch.float32, device=q.device) if return_lse else None
    rc = lib.sage_merge_split(_p(o_part), _p(lse_part), None, None, _p(o), _p(lse), B, S, Hq, group, Lq, D,
                              o_sb, o_sh, o_sl, code, _stream(q))
    _cabi.check(rc, "sage_merge_split")
    return o, lse


def _split_exact_plan(B: int, Hq: int, Lq: int, Lk: int, is_causal: bool, override) -> int:
    """Number of chunks S of the exact split-KV route (``split_kv_exact=True``; 0 = no split).  ``override`` is ``split_kv``: None /
    "auto" = the inexact route's non-causal plan over the floor(Lk / 64) whole tiles (a ragged rest of the key range becomes a tail chunk,
    so a ragged Lk is planned too), and no split for causal calls (dense causal splits measured slower, see :func:`_split_kv_plan`); an
    integer S >= 2 = that split, causal or not, S | floor(Lk / 64); 0 = no split."""
    if override is None:
        override = "auto"
    if override == 0 and not isinstance(override, bool):
        return 0
    ntw = Lk // 64
    if override == "auto":
        return 0 if is_causal else _split_kv_plan(B, Hq, Lq, ntw * 64, False, "auto")
    if isinstance(override, bool) or not isinstance(override, int):
        raise ValueError(f"split_kv={override!r}: 0, an integer >= 2 or 'auto'")
    if override < 2 or override > ntw or ntw % override != 0:
        raise ValueError(f"split_kv={override} with split_kv_exact=True must be >= 2 and divide the number of whole 64-key tiles "
                         f"(kv_len {Lk}: {ntw} tiles)")
    return override


def _split_exact_args(kwargs, qk_quant_gran: str, pv_accum_dtype: str, Lk: int) -> bool:
    """Whether ``split_kv_exact`` asks for the exact split route; its argument errors (checked before any work).  The route exists for the
    default FP8 path only -- fused per-thread Q quantiser, two-level accumulation, the exact score form -- and is never swapped for another
    route behind the caller's back."""
    if not kwargs.get("split_kv_exact", False):
        return False
    if qk_quant_gran != "per_thread" or not kwargs.get("fuse_q_quant", True):
        raise ValueError("split_kv_exact=True needs qk_quant_gran='per_thread' with the fused Q quantiser")
    if pv_accum_dtype == "fp32":
        raise ValueError("split_kv_exact=True needs pv_accum_dtype 'fp32+fp32' or 'fp32+fp16' (two-level accumulation)")
    if ops.fp8_folded(kwargs.get("fp8_scores")):
        raise ValueError("split_kv_exact=True takes the exact score form only (fp8_scores='folded' given)")
    override = kwargs.get("split_kv")
    if override is not None and override != "auto" and not (override == 0 and not isinstance(override, bool)):
        _split_exact_plan(1, 1, 1, Lk, False, override)          # (raises on an S that does not divide the whole tiles)
    return True


def _kv_lens_args(kv_lens, q, tensor_layout, qk_quant_gran: str, pv_accum_dtype: str, smooth_v: bool, kwargs) -> bool:
    """Whether ``kv_lens`` asks for the per-sample key lengths route; its argument errors (checked before any work, on any device).  The route
    exists for the default FP8 path only -- fused per-thread Q quantiser, two-level accumulation, the exact score form, no split -- and, as
    with :func:`_split_exact_args`, is never swapped for another route behind the caller's back: anything else raises ValueError."""
    if kv_lens is None:
        return False
    if not isinstance(kv_lens, torch.Tensor) or kv_lens.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"kv_lens must be an int32 or int64 tensor (got {getattr(kv_lens, 'dtype', type(kv_lens).__name__)})")
    B = q.shape[0]
    if kv_lens.dim() != 1 or kv_lens.shape[0] != B:
        raise ValueError(f"kv_lens must have shape [B] = [{B}] (got {tuple(kv_lens.shape)})")
    if kv_lens.device != q.device:
        raise ValueError(f"kv_lens must be on q's device {q.device} (got {kv_lens.device})")
    _offset_route_restrictions("kv_lens", qk_quant_gran, pv_accum_dtype, smooth_v, kwargs)
    return True


def _pack_gqa_args(pack_gqa, q, k, tensor_layout, qk_quant_gran: str, pv_accum_dtype: str, smooth_v: bool, kwargs) -> bool:
    """Whether ``pack_gqa`` asks for the packed decode launch; its argument errors (checked before any work, on any device).  The launch is one
    of the ``kv_lens`` kernel family, so that route's restrictions hold (:func:`_offset_route_restrictions`), worded for this keyword; it exists
    for decode shapes -- no more query rows than one wave's slab holds -- and needs a GQA group to pack."""
    if pack_gqa is None or pack_gqa is False:
        return False
    if pack_gqa is not True:
        raise ValueError(f"pack_gqa must be None, False or True (got {pack_gqa!r})")
    _offset_route_restrictions("pack_gqa", qk_quant_gran, pv_accum_dtype, smooth_v, kwargs)
    Hq, Lq = _dims(q, tensor_layout)[1:3]
    Hkv = _dims(k, tensor_layout)[1]
    if Lq > 32:
        raise ValueError(f"pack_gqa needs qo_len <= 32 (got {Lq}): a query head's rows are one wave's 32-row slab")
    if Hq == Hkv:
        raise ValueError(f"pack_gqa needs num_qo_heads / num_kv_heads >= 2 (got {Hq} / {Hkv}): there is no GQA group to pack")
    return True


# The auto plan's constants, set from tools/num_splits_probe.py (profiles/num_splits_probe.json):
_NUM_SPLITS_AUTO_MAX_WGS = 64        # the largest unsplit launch a split was faster for (at 128 workgroups and more no chunk count was)
_NUM_SPLITS_AUTO_TARGET = 512        # workgroups the plan aims at: two per compute unit of an MI355X, what the D = 128 kernels keep resident
_NUM_SPLITS_AUTO_MIN_TILES = 8       # no chunk shorter than this many 64-key tiles
_NUM_SPLITS_AUTO_MIN_KEYS, _NUM_SPLITS_AUTO_MAX_KEYS = 8192, 65536      # the shortest and the longest key range measured
_NUM_SPLITS_AUTO_MAX_ROWS = 32       # decode-shaped calls only (measured: 1 and 16 rows; 32 is what one wave's slab and pack_gqa take)
_NUM_SPLITS_AUTO_MIN_S, _NUM_SPLITS_AUTO_MAX_S = 8, 32      # chunk counts that were faster wherever the plan chooses them (2 and 4 are not: pass 1
                                                            # costs about what pass 2 does); 32 is the largest measured


def _num_splits_plan(B: int, Hq: int, Hkv: int, Lq: int, Lk: int, packed: bool) -> int:
    """``num_splits="auto"``: the chunk count from the shapes alone (0 = no split).  No split where the unsplit launch -- ``B * Hkv *
    ceil(group / 4)`` workgroups packed, ``B * Hq`` unpacked -- has more than 64 workgroups, nor below 8192 or above 65536 keys, nor above
    32 query rows; else the smallest S with ``workgroups * S >= 512``, capped so that no chunk is shorter than eight tiles and at 32, and no
    split if that leaves fewer than 8 chunks.  Every choice the plan makes on the probe's shapes is faster there than the unsplit call,
    launches alone and whole call, by more than the measurement's spread.  The probe's shapes are bf16, D 128, GQA 32 / 8, bottom-right
    causal, 1 and 16 rows, B 1 ... 32, 8192 / 32768 / 65536 keys, packed and unpacked: inside those bounds of rows, keys and workgroups the
    plan extrapolates over what it does not see or the probe did not vary -- head size, head ratio, the mask, row and key counts between
    the measured ones -- on the ground that the gain comes from the workgroup count and the chain length alone; outside them it returns no
    split (an explicit ``num_splits=S`` is the caller's to choose anywhere)."""
    wgs = B * Hkv * ((Hq // Hkv + 3) // 4) if packed else B * Hq
    if wgs > _NUM_SPLITS_AUTO_MAX_WGS or not _NUM_SPLITS_AUTO_MIN_KEYS <= Lk <= _NUM_SPLITS_AUTO_MAX_KEYS or Lq > _NUM_SPLITS_AUTO_MAX_ROWS:
        return 0
    tiles = (Lk + 63) // 64
    S = min(-(-_NUM_SPLITS_AUTO_TARGET // wgs), tiles // _NUM_SPLITS_AUTO_MIN_TILES, _NUM_SPLITS_AUTO_MAX_S)
    return S if S >= _NUM_SPLITS_AUTO_MIN_S else 0


def _num_splits_args(num_splits, q, k, tensor_layout, window_size, pack_gqa, qk_quant_gran: str, pv_accum_dtype: str, smooth_v: bool, kwargs) -> int:
    """The chunk count ``num_splits`` asks for (0: none -- ``None`` and ``1`` are the call without the keyword); its argument errors (checked
    before any work, on any device, and in front of the other keywords' checks so that they name this one).  The split is one of the
    ``kv_lens`` kernel family, so that route's restrictions hold (:func:`_offset_route_restrictions`), worded for this keyword; it serves
    calls of one query block and takes no ``window_size`` that bounds the look-back (``left >= 0``; a malformed one is :func:`_window_args`'s
    to refuse).  ``"auto"`` / ``0`` plans from the shapes (:func:`_num_splits_plan`)."""
    if num_splits is None:
        return 0
    auto = isinstance(num_splits, str) and num_splits == "auto"
    if isinstance(num_splits, bool) or not (auto or (isinstance(num_splits, int) and 0 <= num_splits <= 255)):
        raise ValueError(f"num_splits must be None, an int in [0, 255] or 'auto' (got {num_splits!r})")
    if num_splits == 1:
        return 0
    _offset_route_restrictions("num_splits", qk_quant_gran, pv_accum_dtype, smooth_v, kwargs)
    _, Hq, Lq = _dims(q, tensor_layout)[:3]
    B, Hkv, Lk = _dims(k, tensor_layout)[:3]
    if Lq > 128:
        raise ValueError(f"num_splits needs qo_len <= 128 (got {Lq}): the route serves calls of one query block")
    if isinstance(window_size, (tuple, list)) and len(window_size) == 2 and isinstance(window_size[0], int) and window_size[0] >= 0:
        raise ValueError(f"num_splits cannot be combined with window_size={tuple(window_size)!r}: a window that bounds the look-back bounds the keys itself")
    if auto or num_splits == 0:
        return _num_splits_plan(B, Hq, Hkv, Lq, Lk, pack_gqa is True)
    return num_splits


def _window_pair(window_size, is_causal: bool):
    """``window_size`` as the pair ``(left, right)`` (FlashAttention's convention, -1 = unbounded on that side), None when it asks for nothing;
    the argument errors that the dense and the packed route share, worded once."""
    if window_size is None:
        return None
    ok_int = lambda x: isinstance(x, int) and not isinstance(x, bool)
    if not isinstance(window_size, (tuple, list)) or len(window_size) != 2 or not all(ok_int(x) for x in window_size):
        raise ValueError(f"window_size must be a pair of ints (left, right), -1 = unbounded on that side (got {window_size!r})")
    left, right = window_size
    if left < -1 or right < -1:
        raise ValueError(f"window_size=({left}, {right}): a side is -1 (unbounded) or a number of keys >= 0")
    if is_causal and right not in (0, -1):
        raise ValueError(f"window_size=({left}, {right}) with is_causal=True: right must be 0 or -1 (a causal row sees no key behind its diagonal)")
    if left == -1 and (is_causal or right == -1):
        return None                        # unbounded: the call without the keyword
    return left, right


def _window_args(window_size, is_causal: bool, qk_quant_gran: str, pv_accum_dtype: str, smooth_v: bool, kwargs):
    """``window_size=(left, right)`` (FlashAttention's convention, -1 = unbounded on that side) as ``(W, r)``: a row sees ``W`` keys up to and
    including its diagonal (0: unbounded), the diagonal shifted right by ``r`` keys; None when there is no window.  Its argument errors are
    checked before any work, on any device.  A window rides on the ``q_start`` route, so that route's restrictions hold, worded for this
    keyword.  With ``is_causal=False`` and ``right >= 0`` the call runs the causal kernels with the diagonal ``right`` keys further right."""
    pair = _window_pair(window_size, is_causal)
    if pair is None:
        return None
    left, right = pair
    if not is_causal and right == -1:
        raise ValueError(f"window_size=({left}, -1) with is_causal=False: a bounded look-back needs right >= 0 (or is_causal=True)")
    _offset_route_restrictions("window_size", qk_quant_gran, pv_accum_dtype, smooth_v, kwargs)
    r = 0 if is_causal else right
    return (0 if left == -1 else min(left + r + 1, 2 ** 30), r)


def _offset_route_restrictions(what: str, qk_quant_gran: str, pv_accum_dtype: str, smooth_v: bool, kwargs) -> None:
    """What the ``kv_lens`` route asks of a call (:func:`_kv_lens_args`), worded for the keyword ``what`` that rides on it."""
    if qk_quant_gran != "per_thread":
        raise ValueError(f"{what} needs qk_quant_gran='per_thread' (got {qk_quant_gran!r})")
    if not kwargs.get("fuse_q_quant", True):
        raise ValueError(f"{what} needs the fused Q quantiser (fuse_q_quant=False given)")
    if pv_accum_dtype == "fp32":
        raise ValueError(f"{what} needs pv_accum_dtype 'fp32+fp32' or 'fp32+fp16' (two-level accumulation)")
    if ops.fp8_folded(kwargs.get("fp8_scores")):
        raise ValueError(f"{what} takes the exact score form only (fp8_scores='folded' given)")
    if smooth_v:
        raise ValueError(f"{what} does not support smooth_v=True")
    split = kwargs.get("split_kv")
    if split is not None and not (split == 0 and not isinstance(split, bool)):
        raise ValueError(f"{what} cannot be combined with split_kv={split!r} (None or 0 only)")
    if kwargs.get("split_kv_exact", False):
        raise ValueError(f"{what} cannot be combined with split_kv_exact=True")


def _q_start_args(q_start, causal_align: str, is_causal: bool, q, qk_quant_gran: str, pv_accum_dtype: str, smooth_v: bool, kwargs) -> bool:
    """Whether ``q_start`` / ``causal_align`` ask for per-sample query offsets; their argument errors (checked before any work, on any
    device).  The offsets ride on the ``kv_lens`` route, so its restrictions hold (:func:`_kv_lens_args`), worded for these keywords."""
    if causal_align not in ("top_left", "bottom_right"):
        raise ValueError(f"causal_align must be 'top_left' or 'bottom_right' (got {causal_align!r})")
    if q_start is None and causal_align == "top_left":
        return False
    what = "q_start" if q_start is not None else "causal_align='bottom_right'"
    if q_start is not None and causal_align != "top_left":
        raise ValueError("pass either q_start or causal_align='bottom_right' (which is q_start = clamp(kv_lens, 0, kv_len) - qo_len), not both")
    if not is_causal:
        raise ValueError(f"{what} needs is_causal=True (it places the causal diagonal)")
    B = q.shape[0]
    if q_start is not None and not (isinstance(q_start, int) and not isinstance(q_start, bool)):
        if not isinstance(q_start, torch.Tensor) or q_start.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"q_start must be an int or an int32 / int64 tensor (got {getattr(q_start, 'dtype', type(q_start).__name__)})")
        if q_start.dim() != 1 or q_start.shape[0] != B:
            raise ValueError(f"q_start must have shape [B] = [{B}] (got {tuple(q_start.shape)})")
        if q_start.device != q.device:
            raise ValueError(f"q_start must be on q's device {q.device} (got {q_start.device})")
    _offset_route_restrictions(what, qk_quant_gran, pv_accum_dtype, smooth_v, kwargs)
    return True


def _q_start_tensor(q_start, kv_lens, B: int, Lq: int, Lk: int, device, shift: int = 0) -> torch.Tensor:
    """The int32 ``[B]`` offsets of the attention call, formed on the device (no host read): the caller's tensor, an int broadcast to the
    batch, or -- ``q_start`` None: ``causal_align='bottom_right'`` -- ``clamp(kv_lens, 0, Lk) - Lq``.  ``shift`` (``window_size``'s ``right``
    of a non-causal call: the diagonal moved right) is added to them, saturating at int32's end."""
    if shift:
        s = _q_start_tensor(q_start, kv_lens, B, Lq, Lk, device)
        return (s.to(torch.int64) + int(shift)).clamp(max=2 ** 31 - 1).to(torch.int32)
    if q_start is None:
        if kv_lens is None:
            return torch.full((B,), Lk - Lq, dtype=torch.int32, device=device)
        return (kv_lens.clamp(0, Lk) - Lq).to(torch.int32).contiguous()
    if isinstance(q_start, int):
        return torch.full((B,), max(-2 ** 31, min(2 ** 31 - 1, q_start)), dtype=torch.int32, device=device)
    if q_start.dtype == torch.int64:       # (offsets outside int32 are far outside [-Lq, Lk] either way: clamp before narrowing)
        q_start = q_start.clamp(-2 ** 31, 2 ** 31 - 1)
    return q_start.to(torch.int32).contiguous()


class _KvFamily(NamedTuple):
    """What the keywords of the ``kv_lens`` kernel family ask of a call (:func:`_kv_family_args`)."""
    is_causal: bool        # the call's, or True under a window
    window: int            # keys a row sees up to and including its diagonal (0: unbounded)
    shift: int             # keys the diagonal lies further right (a non-causal window's ``right``)
    gqa_pack: bool
    splits: int            # key-range chunks (0: none)
    with_lens: bool
    with_start: bool
    q_start: Any           # the caller's, or 0 under a window without offsets


def _kv_family_args(q, k, tensor_layout, is_causal: bool, kv_lens, q_start, causal_align: str, window_size, pack_gqa, num_splits,
                    qk_quant_gran: str, pv_accum_dtype: str, smooth_v: bool, kwargs) -> _KvFamily:
    """The keywords of the ``kv_lens`` kernel family, resolved for ``sageattn_qk_int8_pv_fp8_cuda`` and ``sageattn_kvcache`` alike (``k``: K or
    the cache's INT8 K, for its shape; the cache, which has no ``kv_lens`` keyword, passes None).  Their argument errors, checked before any
    work and on any device, in this order: ``num_splits``, ``pack_gqa``, ``kv_lens``, ``window_size``, ``q_start`` / ``causal_align`` -- a
    call that breaks two keywords' rules gets the earlier one's error, and a restriction of the route is worded for the first keyword that
    asks for the route."""
    route = (qk_quant_gran, pv_accum_dtype, smooth_v, kwargs)
    splits = _num_splits_args(num_splits, q, k, tensor_layout, window_size, pack_gqa, *route)
    gqa_pack = _pack_gqa_args(pack_gqa, q, k, tensor_layout, *route)
    with_lens = _kv_lens_args(kv_lens, q, tensor_layout, *route)
    win = _window_args(window_size, is_causal, *route)
    window, shift = win if win is not None else (0, 0)
    if win is not None:                    # the causal kernels, the diagonal `shift` keys further right; offsets 0 unless the caller places the rows
        is_causal = True
        if q_start is None and causal_align == "top_left":
            q_start = 0
    with_start = _q_start_args(q_start, causal_align, is_causal, q, *route)
    return _KvFamily(is_causal, window, shift, gqa_pack, splits, with_lens, with_start, q_start)


def _attn_kv_family(call: _KvFamily, q, lens, kv_lens, k_int8, v_image, v_scale, k_scale, tensor_layout, sm_scale, return_lse, head_dim_og,
                    smooth_k, lse_correction, paged=None):
    """The attention of a call on the ``kv_lens`` entry, from its resolved keywords and quantised operands: ``lens`` are the int32 lengths the
    kernel reads, ``kv_lens`` what ``causal_align='bottom_right'`` forms its offsets from (None: the padded key length).  ``paged``: the
    ``PagedQuantizedKVCache`` whose pool the operands are (its ``capacity`` is then the padded key length).  Nothing here reads a length or an
    offset on the host."""
    B, _, Lq = _dims(q, tensor_layout)[:3]
    Lk = paged.capacity if paged is not None else _dims(k_int8, tensor_layout)[2]
    start = _q_start_tensor(call.q_start, kv_lens, B, Lq, Lk, q.device, call.shift) if call.with_start else None
    o, lse = _attn_fused_q(_aligned(q, 8), k_int8, v_image, v_scale, k_scale, tensor_layout, call.is_causal, _sm_log2(sm_scale), return_lse,
                           kv_lens=lens, q_start=start, window=call.window, gqa_pack=call.gqa_pack, num_splits=call.splits, paged=paged)
    return _finish(o, lse, head_dim_og, return_lse, smooth_k, lse_correction, sm_scale)


@torch.compiler.disable
def _attn_fused_q_split_exact(q, k_int8, v_image, v_scale, k_scale, tensor_layout, is_causal, sm_scale_log2, S, return_lse, v_mean=None):
    """Exact split-KV route of the fused-Q FP8 attention: pass 1 (``sage_split_exact_chunk_max``) computes every chunk's row maxima with
    the attention kernel's arithmetic, pass 2 (``sage_attn_fused_q_pv_f8_split_exact``) runs the S chunks of floor(Lk / 64) / S whole tiles
    with their running maximum started at the unsplit call's -- so every P is the unsplit call's -- into FP32 partials, a second launch
    runs a ragged tail of the key range seeded with the maximum over all chunks, and ``sage_merge_split_f32`` merges them.  The operands
    of the unsplit call are read in place; no host synchronisation."""
    B, Hq, Lq, D, q_sb, q_sh, q_sl = _dims(q, tensor_layout)
    _, Hkv, Lk, _, k_sb, k_sh, k_sl = _dims(k_int8, tensor_layout)
    group = Hq // Hkv
    assert v_image.is_contiguous() and k_scale.is_contiguous() and v_scale.is_contiguous()
    assert k_scale.shape[-1] == ((Lk + 63) // 64) * 4, "per-thread k scales of 64-key tiles"
    dev = q.device
    chunk_max = torch.empty((B, Hq * S, Lq), dtype=torch.float32, device=dev)
    o_part = torch.empty((B, Hq * S, Lq, D), dtype=torch.float32, device=dev)
    lse_part = torch.empty((B, Hq * S, Lq), dtype=torch.float32, device=dev)
    code = _cabi.DTYPE_F16 if q.dtype == torch.float16 else _cabi.DTYPE_BF16
    lib, stream = _cabi.load(), _stream(q)
    rc = lib.sage_split_exact_chunk_max(_p(q), _p(k_int8), _p(k_scale), _p(chunk_max), B, Hq, Hkv, S, Lq, Lk, D,
                                        q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, int(is_causal), float(sm_scale_log2), code, stream)
    _cabi.check(rc, "sage_split_exact_chunk_max")
    o_tail = lse_tail = None
    for tail in (0, 1) if Lk % 64 else (0,):
        if tail:
            o_tail = torch.empty((B, Hq, Lq, D), dtype=torch.float32, device=dev)
            lse_tail = torch.empty((B, Hq, Lq), dtype=torch.float32, device=dev)
        rc = lib.sage_attn_fused_q_pv_f8_split_exact(
            _p(q), _p(k_int8), _p(v_image), _p(o_tail if tail else o_part), _p(lse_tail if tail else lse_part), _p(k_scale), _p(v_scale),
            _p(v_mean), _p(chunk_max), B, Hq, Hkv, S, tail, Lq, Lk, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl,
            int(is_causal), float(sm_scale_log2), code, stream, None)
        _cabi.check(rc, "sage_attn_fused_q_pv_f8_split_exact")
    o = torch.empty(q.shape, dtype=q.dtype, device=dev)
    _, _, _, _, o_sb, o_sh, o_sl = _dims(o, tensor_layout)
    lse = torch.empty((B, Hq, Lq), dtype=torch.float32, device=dev) if return_lse else None
    rc = lib.sage_merge_split_f32(_p(o_part), _p(lse_part), _p(o_tail), _p(lse_tail), _p(o), _p(lse), B, S, Hq, group, Lq, D,
                                  o_sb, o_sh, o_sl, code, stream)
    _cabi.check(rc, "sage_merge_split_f32")
    return o, lse


@torch.compiler.disable
def _attn_masked(q_int8, k_int8, v_image, q_scale, k_scale, attn_mask, out_dtype, tensor_layout, return_lse):
    """Triton-named API with ``attn_mask`` (core.py:313-324): the mask is broadcast to
    ``[B, Hq, Lq, Lk]`` by ``expand`` (zero strides, no copy) and read in place by the kernel."""
    B, Hq, Lq, D, q_sb, q_sh, q_sl = _dims(q_int8, tensor_layout)
    _, Hkv, Lk, _, k_sb, k_sh, k_sl = _dims(k_int8, tensor_layout)
    assert Hq % Hkv == 0, "num_qo_heads must be divisible by num_kv_heads"
    target_shape = (B, Hq, Lq, Lk)
    try:
        attn_mask = attn_mask.expand(target_shape)
    except Exception:
        raise AssertionError(f"attn_mask shape {attn_mask.shape} cannot be broadcast to {target_shape}")
    kind = _cabi.MASK_BOOL if attn_mask.dtype == torch.bool else (_cabi.MASK_F16 if attn_mask.dtype == torch.float16 else _cabi.MASK_BF16)
    o = torch.empty(q_int8.shape, dtype=out_dtype, device=q_int8.device)
    _, _, _, _, o_sb, o_sh, o_sl = _dims(o, tensor_layout)
    lse = torch.empty((B, Hq, Lq), dtype=torch.float32, device=o.device) if return_lse else None
    code = _cabi.DTYPE_F16 if out_dtype == torch.float16 else _cabi.DTYPE_BF16
    rc = _cabi.load().sage_attn_qk_int8_pv_f16_masked(
        _p(q_int8), _p(k_int8), _p(v_image), _p(o), _p(lse), _p(q_scale), _p(k_scale), _p(attn_mask), kind,
        attn_mask.stride(0), attn_mask.stride(1), attn_mask.stride(2), attn_mask.stride(3),
        B, Hq, Hkv, Lq, Lk, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, o_sb, o_sh, o_sl, 1.0, code, _stream(o), None)
    _cabi.check(rc, "sage_attn_qk_int8_pv_f16_masked")
    return o, lse


def _finish(o, lse, head_dim_og, return_lse, smooth_k, lse_correction, sm_scale):
    o = o[..., :head_dim_og]
    if return_lse:   # core.py:328-329: kernel LSE is in log2 units
        return o, lse / 1.44269504 + lse_correction * sm_scale if smooth_k else lse / 1.44269504
    return o


def _refuse_kv_family_compiled(kv_lens, q_start, causal_align, window_size, pack_gqa, num_splits, why: str = "") -> None:
    """The compiled op has no argument for the ``kv_lens`` family's keywords: a compiled call that ignored one would be a trap."""
    for what, given in (("kv_lens is", kv_lens is not None),
                        ("q_start / causal_align are", q_start is not None or causal_align != "top_left"),
                        ("window_size is", window_size is not None),
                        ("pack_gqa is", pack_gqa),
                        ("num_splits is", num_splits is not None and num_splits != 1)):
        if given:
            raise ValueError(f"{what} not supported under torch.compile{why}")


# ------------------------------------------------------------------------------------------------
def sageattn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tensor_layout: str = "HND", is_causal: bool = False,
             sm_scale: Optional[float] = None, return_lse: bool = False, kv_lens: Optional[torch.Tensor] = None, q_start=None,
             causal_align: str = "top_left", window_size=None, pack_gqa=None, num_splits=None, **kwargs: Any):
    """Select the implementation for the device, as the reference does per compute capability
    (core.py:143-157).  On gfx950 that is INT8 QK^T + FP8 PV with two-level FP32 accumulation
    (the reference's sm90 choice, ``pv_accum_dtype="fp32+fp32"``).  Extra SDPA-style kwargs
    (``attn_mask=``, ``dropout_p=``, ``scale=`` ...) are accepted and ignored exactly as the
    reference ignores them.  ``kv_lens`` (gfx950 extension, int32 / int64 ``[B]`` on q's device): a key length per sample of a right-padded
    batch; ``q_start`` (int, or int32 / int64 ``[B]``) / ``causal_align="bottom_right"``: where the causal diagonal of each sample lies -- row i
    attends to key j iff ``j <= q_start[b] + i`` and ``j < len_b``; ``window_size=(left, right)``: a sliding window in FlashAttention's
    convention; ``pack_gqa=True``: a decode-shaped call (``qo_len <= 32``) runs a GQA group's query heads four to a workgroup, same bits;
    ``num_splits=S`` / ``"auto"``: a call of one query block (``qo_len <= 128``) runs as S key-range chunks, exactly.
    See :func:`sageattn_qk_int8_pv_fp8_cuda`."""
    _check_shapes(q, k, v, tensor_layout)      # (again in the entry point called below: this one is in front of the device query)
    if torch.compiler.is_compiling():      # the device query is not traceable; the opaque op checks the device when it runs
        _refuse_kv_family_compiled(kv_lens, q_start, causal_align, window_size, pack_gqa, num_splits)
        return sageattn_qk_int8_pv_fp8_cuda(q, k, v, tensor_layout=tensor_layout, is_causal=is_causal, sm_scale=sm_scale,
                                            return_lse=return_lse, pv_accum_dtype="fp32+fp32")
    arch = get_gcn_arch(q.device) if q.is_cuda else "cpu"
    if arch.startswith(_SUPPORTED_ARCH_PREFIX):
        return sageattn_qk_int8_pv_fp8_cuda(q, k, v, tensor_layout=tensor_layout, is_causal=is_causal, sm_scale=sm_scale,
                                            return_lse=return_lse, pv_accum_dtype="fp32+fp32", split_kv=kwargs.get("split_kv"),
                                            fused_prepass=kwargs.get("fused_prepass"), fp8_scores=kwargs.get("fp8_scores"),
                                            split_kv_exact=kwargs.get("split_kv_exact", False), kv_lens=kv_lens,
                                            q_start=q_start, causal_align=causal_align, window_size=window_size, pack_gqa=pack_gqa,
                                            num_splits=num_splits)
    raise ValueError(f"Unsupported architecture: {arch} (sageattention_amd targets gfx950 / MI355X only)")


def sageattn_qk_int8_pv_fp16_triton(q, k, v, tensor_layout: str = "HND", quantization_backend: str = "triton",
                                    is_causal: bool = False, attn_mask: Optional[torch.Tensor] = None,
                                    sm_scale: Optional[float] = None, smooth_k: bool = True, return_lse: bool = False,
                                    **kwargs: Any):
    """Per-block INT8 Q/K (sm_scale*log2e folded into Q), FP16 PV, per-tile product added to an
    FP32 buffer (reference core.py:160-331; the name is kept for drop-in -- there is no Triton
    here, the same HIP kernel family runs it)."""
    dtype = q.dtype
    _check_inputs(q, k, v)
    _check_shapes(q, k, v, tensor_layout)
    if attn_mask is not None:
        assert attn_mask.dtype == torch.bool or attn_mask.dtype == q.dtype, "attn_mask must be of dtype bool or the same dtype as q."
        assert attn_mask.device == q.device, "All tensors must be on the same device."
    if quantization_backend not in ("triton", "cuda"):
        raise ValueError(f"Unsupported quantization backend: {quantization_backend}")
    torch.cuda.set_device(v.device)
    q, k, v, head_dim_og = _pad_head_dim(q, k, v)
    assert q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1, "Last dim of qkv must be contiguous."
    # the Q half of the per-block quantiser runs in the attention kernel's prologue (same bits, no INT8 copy of Q in HBM) unless the
    # CUDA rounding convention or a mask is asked for; fp16 inputs on that route need no V pass at all: the kernel reads V's rows in place
    # (the reference's `v.to(torch.float16)`, core.py:297-298, is the identity for them) -- same bits as the image route
    fuse_q = quantization_backend == "triton" and attn_mask is None and kwargs.get("fuse_q_quant", True)
    v_rows = fuse_q and _v_rows_wanted(q, k, v, tensor_layout, is_causal, kwargs.get("v_in_place"))
    # K mean + INT8 K (Triton rounding) + the fp16 V image as ONE launch that reads K and V once (sage_prepass_kv), when it is the faster route
    k_done = v_image = None
    if quantization_backend == "triton" and _fused_prepass_wanted(k, tensor_layout, kwargs.get("fused_prepass")):
        km_s, k8, ks, v_image, _, _ = prepass_kv_fp8(k, None if v_rows else v, tensor_layout, smooth_k=smooth_k, qk_quant_gran="per_block_triton",
                                                     v_fp16=True)
        k_done = (k8, ks)
        km, lse_correction = None, None
        if smooth_k:
            km = km_s.unsqueeze(1 if tensor_layout == "NHD" else 2)
            lse_correction = _lse_correction(q, km, tensor_layout) if return_lse else None
    else:
        km, lse_correction = _smooth_k(q, k, tensor_layout, smooth_k, return_lse)
    if sm_scale is None:
        sm_scale = 1.0 / (head_dim_og ** 0.5)
    if is_causal:
        assert q.size(1 if tensor_layout == "NHD" else 2) == k.size(1 if tensor_layout == "NHD" else 2), \
            "qo_len and kv_len must be equal for causal attention"
    if is_causal:
        assert attn_mask is None, "Mask should be None for causal attention."        # core.py:310
    q_int8, q_scale, k_int8, k_scale = per_block_int8(None if fuse_q else q, k, km=km, sm_scale=sm_scale, tensor_layout=tensor_layout,
                                                      quantization_backend=quantization_backend, k_done=k_done)
    if v_image is None and not v_rows:
        v_image = prep_v_fp16(v, tensor_layout)
    if fuse_q:
        o, lse = _attn_fused_qblock(q, k_int8, v if v_rows else v_image, k_scale, tensor_layout, is_causal, sm_scale * LOG2E, return_lse, v_rows=v_rows)
    elif attn_mask is not None:
        o, lse = _attn_masked(q_int8, k_int8, v_image, q_scale, k_scale, attn_mask, dtype, tensor_layout, return_lse)
    else:
        o, lse = _attn_dense(False, q_int8, k_int8, v_image, None, q_scale, k_scale, dtype, tensor_layout, is_causal,
                             _cabi.GRAN_PER_BLOCK, 128, 1.0, "triton", return_lse)
    return _finish(o, lse, head_dim_og, return_lse, smooth_k, lse_correction, sm_scale)


class _VarlenState:
    """Operands of the attention launch of one ``sageattn_varlen`` call (what its pre-pass produces)."""
    __slots__ = ("q", "q_int8", "q_scale", "k_int8", "k_scale", "v_image", "cu_q", "cu_k", "cu_qs", "cu_ks", "order", "plan", "fuse_q",
                 "max_seqlen_q", "is_causal", "q_premul", "dtype", "head_dim_og", "v_scale", "km", "sm_scale", "bottom_right", "window")


@torch.compiler.disable
def _varlen_prepare(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal, sm_scale, smooth_k, kwargs,
                    v_fp8: bool = False, bottom_right: bool = False, window: int = 0) -> _VarlenState:
    """Everything of ``sageattn_varlen`` in front of the attention launch (core.py:427-444): the index arrays (one launch, no host
    synchronisation), ``km`` over all packed tokens, INT8 K, the fp16 V image -- one launch that reads K and V once where the head barrier
    reaches (``prepass_kv_varlen``), else the kernel sequence with the same bits.  ``v_fp8`` (``sageattn_qk_int8_pv_fp8_varlen``): the same
    Q / K half, and V as the e4m3 image with per-(sequence, head, channel) scales (``per_channel_fp8_varlen``) instead of the fp16 image."""
    st = _VarlenState()
    st.dtype = q.dtype
    _check_inputs(q, k, v)
    _check_shapes(q, k, v, None, cu_seqlens_q, cu_seqlens_k)
    torch.cuda.set_device(v.device)
    q, k, v, st.head_dim_og = _pad_head_dim(q, k, v)
    assert q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1, "Last dim of qkv must be contiguous."
    assert cu_seqlens_q.is_contiguous() and cu_seqlens_k.is_contiguous(), "cu_seqlens_q and cu_seqlens_k must be contiguous."
    Hq, Hkv, D = q.shape[1], k.shape[1], q.shape[2]
    assert Hq % Hkv == 0, "num_qo_heads must be divisible by num_kv_heads"
    if sm_scale is None:
        sm_scale = 1.0 / (st.head_dim_og ** 0.5)
    st.sm_scale = sm_scale
    st.fuse_q = fuse_q = kwargs.get("fuse_q_quant", True)      # the Q half of the quantiser in the attention kernel's prologue (same bits)
    st.cu_q = cu_q = cu_seqlens_q.to(torch.int32).contiguous()
    st.cu_k = cu_k = cu_seqlens_k.to(torch.int32).contiguous()
    nseq = cu_q.shape[0] - 1
    # block-count prefix sums, the attention launch's work list and the pre-pass's slab map from one small launch (None: more sequences than
    # it takes -- then torch prefix sums, an on-device argsort for the order and the kernel sequence)
    # (bottom-right alignment: the work list is sorted by the weights of that mask -- sage_varlen_plan's is_causal = 2; a window on top of it
    #  keeps that order, the unwindowed one: results never depend on it, and everything else in front of the launch is the unwindowed call's)
    st.bottom_right = bool(bottom_right)
    st.window = int(window)
    plan = varlen_plan(cu_q, cu_k, want_q_blocks=not fuse_q, total_q=q.shape[0], total_k=k.shape[0], is_causal=2 if bottom_right else is_causal,
                       Hq=Hq, Hkv=Hkv, head_dim=D, pv_fp8=v_fp8) if kwargs.get("varlen_plan", True) else None
    st.plan = plan if (plan is not None and kwargs.get("work_list", True)) else None
    fused = kwargs.get("fused_prepass")
    if fused is None:
        fused = os.environ.get("SAGE_PREPASS", "") not in ("seq", "sequence", "0")
    fused = bool(fused) and prepass_varlen_fused_ok(k, plan, max_seqlen_k, smooth_k)
    st.v_scale = None
    if fused:
        st.km, st.k_int8, st.k_scale, st.v_image = prepass_kv_varlen(k, None if v_fp8 else v, cu_k, plan, max_seqlen_k, smooth_k=smooth_k)
        st.cu_ks = plan.cu_ks
        st.q_int8 = st.q_scale = st.cu_qs = None
        if not fuse_q:
            st.q_int8, st.q_scale, _, _, st.cu_qs, _ = per_block_int8_varlen(q, None, cu_q, cu_k, max_seqlen_q, max_seqlen_k, sm_scale=sm_scale,
                                                                            cu_qs=plan.cu_qs)
    else:
        st.km = km = channel_mean_packed(k, cu_k, plan) if smooth_k else None   # mean over ALL packed tokens, as core.py:432-434
        # (prefix arrays from the plan, or from torch ops on the device: either way the scale tensors are allocated at their host-known
        #  bounds and nothing synchronises -- the reference's `.item()` pair is gone on every route)
        st.q_int8, st.q_scale, st.k_int8, st.k_scale, st.cu_qs, st.cu_ks = per_block_int8_varlen(
            None if fuse_q else q, k, cu_q, cu_k, max_seqlen_q, max_seqlen_k, km=km, sm_scale=sm_scale,
            cu_ks=plan.cu_ks if plan is not None else _cu_blocks(cu_k, 64),
            cu_qs=None if fuse_q else (plan.cu_qs if plan is not None else _cu_blocks(cu_q, 128)))
        if not v_fp8:
            st.v_image = prep_v_fp16_varlen(v, cu_k, st.cu_ks, max_seqlen_k, ntiles=(k.shape[0] + 63) // 64 + nseq)
    if v_fp8:
        st.v_image, st.v_scale = per_channel_fp8_varlen(v, cu_k, st.cu_ks, max_seqlen_k, plan=plan, ntiles=(v.shape[0] + 63) // 64 + nseq)
    # without a work list: schedule the longest sequences first (on the device, no sync); results do not depend on the order
    st.order = plan.order if plan is not None else torch.argsort(cu_q[1:] - cu_q[:-1], descending=True).to(torch.int32)
    st.q = _aligned(q, 8) if fuse_q else None
    st.max_seqlen_q, st.is_causal, st.q_premul = int(max_seqlen_q), bool(is_causal), float(sm_scale * LOG2E)
    return st


@torch.compiler.disable
def _varlen_attend(st: _VarlenState) -> torch.Tensor:
    """The attention launch of ``sageattn_varlen`` (attn_qk_int8_block_varlen.py:123, _causal_varlen.py:125)."""
    q = st.q if st.fuse_q else st.q_int8
    Hq, D = q.shape[1], q.shape[2]
    Hkv = st.k_int8.shape[1]
    o = torch.empty(q.shape, dtype=st.dtype, device=q.device)
    code = _cabi.DTYPE_F16 if st.dtype == torch.float16 else _cabi.DTYPE_BF16
    plan = st.plan
    items, hdr, bound = (plan.items, plan.hdr, plan.items_bound) if plan is not None else (None, None, 0)
    nseq = st.cu_q.shape[0] - 1
    # (a large call over the work list runs as a persistent launch -- causal too, on the fused-Q route whose causal kernels carry the ticket
    #  loop; items = 128-row blocks of the packed rows, at least)
    attr = ops.attn_attr(q.device, st.is_causal, Hq * (q.shape[0] // 128), packed=st.fuse_q) if plan is not None else None
    if st.fuse_q:
        rc = _cabi.load().sage_attn_fused_qblock_pv_f16_varlen(
            _p(q), _p(st.k_int8), _p(st.v_image), _p(o), _p(st.k_scale), _p(st.cu_q), _p(st.cu_k), _p(st.cu_ks), _p(st.order),
            _p(items), _p(hdr), bound, nseq, st.max_seqlen_q, Hq, Hkv, D, q.stride(0), q.stride(1), st.k_int8.stride(0), st.k_int8.stride(1),
            o.stride(0), o.stride(1), int(st.is_causal), st.q_premul, code, code, _stream(o), _cabi.attr_arg(attr))
        ops.attn_check(rc, "sage_attn_fused_qblock_pv_f16_varlen", attr, q.device)
    else:
        rc = _cabi.load().sage_attn_qk_int8_pv_f16_varlen(
            _p(q), _p(st.k_int8), _p(st.v_image), _p(o), _p(st.q_scale), _p(st.k_scale), _p(st.cu_q), _p(st.cu_k), _p(st.cu_qs), _p(st.cu_ks),
            _p(st.order), _p(items), _p(hdr), bound, nseq, st.max_seqlen_q, Hq, Hkv, D, q.stride(0), q.stride(1),
            st.k_int8.stride(0), st.k_int8.stride(1), o.stride(0), o.stride(1), int(st.is_causal), 1.0, _cabi.PV_ACCUM_TRITON, code, _stream(o),
            _cabi.attr_arg(attr))
        ops.attn_check(rc, "sage_attn_qk_int8_pv_f16_varlen", attr, q.device)
    return o[..., :st.head_dim_og]


@torch.compiler.disable
def sageattn_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q: int, max_seqlen_k: int, is_causal: bool = False,
                    sm_scale: Optional[float] = None, smooth_k: bool = True, **kwargs: Any) -> torch.Tensor:
    """Variable-length batches, q/k/v packed as ``[sum L, H, D]`` (reference core.py:334-448).  Three launches and no host
    synchronisation on the default route: the index arrays (``sage_varlen_plan``), the K / V pre-pass (``sage_prepass_kv_varlen``) and
    the attention kernel over a device-built work list (every workgroup one existing query block, heaviest first) with the per-block Q
    quantisation in its prologue.  Route switches (same bits either way): ``fused_prepass=False`` the kernel sequence,
    ``work_list=False`` the unit order sized by ``max_seqlen_q``, ``fuse_q_quant=False`` a separate Q quantiser; ``varlen_plan=False`` builds
    the index arrays with torch ops as for more than 1024 sequences (the K mean is then summed over packed 512-token slabs instead of
    per-sequence ones: equal up to the last bit of an input-dtype rounding)."""
    return _varlen_attend(_varlen_prepare(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal, sm_scale, smooth_k,
                                          kwargs))


@torch.compiler.disable
def _varlen_attend_f8(st: _VarlenState, two_level: bool, return_lse: bool):
    """The attention launch of ``sageattn_qk_int8_pv_fp8_varlen``: ``_varlen_attend``'s, with the e4m3 V image and its scales, the FP8
    accumulation asked for and the packed LSE ``[Hq, sum Lq]`` (log2 units) when asked for."""
    q = st.q if st.fuse_q else st.q_int8
    T, Hq, D = q.shape
    Hkv = st.k_int8.shape[1]
    o = torch.empty(q.shape, dtype=st.dtype, device=q.device)
    lse = torch.empty((Hq, T), dtype=torch.float32, device=q.device) if return_lse else None
    code = _cabi.DTYPE_F16 if st.dtype == torch.float16 else _cabi.DTYPE_BF16
    accum = _cabi.PV_ACCUM_TWO_LEVEL if two_level else _cabi.PV_ACCUM_SINGLE
    plan = st.plan
    items, hdr, bound = (plan.items, plan.hdr, plan.items_bound) if plan is not None else (None, None, 0)
    nseq = st.cu_q.shape[0] - 1
    # (the bottom-right flag travels in the attributes, with the work list's ticket block or -- no work list: the hardware's dispatch -- alone)
    # (so does the window, a Python int: SageLaunchAttr.window, honoured together with the flag only)
    attr = ops.attn_attr(q.device, st.is_causal, Hq * (T // 128), packed=st.fuse_q, causal_bottom_right=st.bottom_right, window=st.window) \
        if plan is not None else _cabi.launch_attr(causal_bottom_right=st.bottom_right, window=st.window)
    if st.fuse_q:
        rc = _cabi.load().sage_attn_fused_qblock_pv_f8_varlen(
            _p(q), _p(st.k_int8), _p(st.v_image), _p(o), _p(lse), _p(st.k_scale), _p(st.v_scale), _p(st.cu_q), _p(st.cu_k), _p(st.cu_ks),
            _p(st.order), _p(items), _p(hdr), bound, nseq, st.max_seqlen_q, Hq, Hkv, D, q.stride(0), q.stride(1), st.k_int8.stride(0),
            st.k_int8.stride(1), o.stride(0), o.stride(1), T, int(st.is_causal), st.q_premul, accum, code, code, _stream(o), _cabi.attr_arg(attr))
        ops.attn_check(rc, "sage_attn_fused_qblock_pv_f8_varlen", attr, q.device)
    else:
        rc = _cabi.load().sage_attn_qk_int8_pv_f8_varlen(
            _p(q), _p(st.k_int8), _p(st.v_image), _p(o), _p(lse), _p(st.q_scale), _p(st.k_scale), _p(st.v_scale), _p(st.cu_q), _p(st.cu_k),
            _p(st.cu_qs), _p(st.cu_ks), _p(st.order), _p(items), _p(hdr), bound, nseq, st.max_seqlen_q, Hq, Hkv, D, q.stride(0), q.stride(1),
            st.k_int8.stride(0), st.k_int8.stride(1), o.stride(0), o.stride(1), T, int(st.is_causal), 1.0, accum, code, _stream(o),
            _cabi.attr_arg(attr))
        ops.attn_check(rc, "sage_attn_qk_int8_pv_f8_varlen", attr, q.device)
    return o[..., :st.head_dim_og], lse


def _varlen_window_args(window_size, is_causal: bool, causal_align: str, pv_accum_dtype: str, max_seqlen_q, max_seqlen_k, kwargs) -> int:
    """``window_size=(left, right)`` of ``sageattn_qk_int8_pv_fp8_varlen`` as ``W``, the keys a row sees up to and including its bottom-right
    diagonal (0: no window).  The checks it shares with :func:`_window_args` are :func:`_window_pair`'s; the packed route's own restrictions
    behind them.  Checked before any work, on any device."""
    pair = _window_pair(window_size, is_causal)
    if pair is None:
        return 0
    left, right = pair
    if not is_causal:
        raise ValueError(f"window_size=({left}, {right}) with is_causal=False is not supported on packed batches (the packed route has no operand "
                         f"for the diagonal's shift): is_causal=True with right 0 or -1")
    if causal_align != "bottom_right":
        raise ValueError(f'window_size=({left}, {right}) needs causal_align="bottom_right": packed windows are bottom-right aligned (FlashAttention\'s '
                         f'varlen convention); for sequences with Lq = Lk the two alignments coincide (got causal_align={causal_align!r})')
    if pv_accum_dtype != "fp32+fp32":
        raise ValueError(f'window_size needs pv_accum_dtype="fp32+fp32" (got {pv_accum_dtype!r})')
    if not kwargs.get("fuse_q_quant", True):
        raise ValueError("window_size needs the fused Q quantiser (fuse_q_quant=False given)")
    if int(max_seqlen_q) + int(max_seqlen_k) > 2 ** 29:
        raise ValueError(f"window_size: max_seqlen_q + max_seqlen_k must not exceed 2**29 (got {max_seqlen_q} + {max_seqlen_k})")
    return min(left + 1, 2 ** 30)


@torch.compiler.disable
def sageattn_qk_int8_pv_fp8_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q: int, max_seqlen_k: int, is_causal: bool = False,
                                   sm_scale: Optional[float] = None, smooth_k: bool = True, pv_accum_dtype: str = "fp32+fp32",
                                   return_lse: bool = False, **kwargs: Any):
    """Variable-length batches with FP8 (e4m3) PV: ``sageattn_varlen``'s packed ``[sum L, H, D]`` inputs, GQA, head-dim padding, causal
    masking and Q / K half bit for bit (per-block INT8, Triton rounding, sm_scale log2(e) folded into Q, K smoothed by the mean over ALL
    packed tokens), and V in e4m3 with one scale per (sequence, kv-head, channel) -- an outlier token costs no other sequence its V precision.
    ``pv_accum_dtype`` "fp32+fp32" (two-level accumulation) or "fp32" (single level); the exact score form.  ``return_lse``: ``(o, lse)``
    with ``lse`` fp32 ``[Hq, sum Lq]`` in natural-log units, smooth_k corrected as the dense calls' (core.py:328-329).  Route switches as
    ``sageattn_varlen``'s (``fuse_q_quant``, ``work_list``, ``varlen_plan``, ``fused_prepass``): the same bits either way.  No host
    synchronisation on any route.
    ``causal_align`` (a keyword taken from ``kwargs`` by name -- the function's parameter list is pinned by tests/test_varlen_fp8_host.py -- and
    validated here, before any device call): "top_left", the default (the reference's mask: row i of a sequence sees keys j <= i), or
    "bottom_right" (row i of sequence b sees keys j <= i + Lk_b - Lq_b, the lengths from ``cu_seqlens``: the last row sees every key, as
    FlashAttention's varlen call aligns its mask -- chunks of prefill against a cached prefix, decode rows, speculative verification and full prefills in one packed call).  "bottom_right" needs
    ``is_causal=True``, ``pv_accum_dtype="fp32+fp32"`` and the fused Q quantiser; rows in front of key 0 (the first ``Lq_b - Lk_b`` rows of a
    sequence with more rows than keys, every row of one without keys) give ``o = +0`` and ``lse = -inf``.
    ``window_size=(left, right)`` (taken from ``kwargs`` by name as well; FlashAttention's varlen convention, -1 = unbounded on that side): a
    sliding window aligned bottom-right -- with ``W = left + 1`` row i of sequence b sees key j iff ``i + Lk_b - Lq_b - W < j <= i + Lk_b - Lq_b``
    and ``0 <= j < Lk_b``; tiles in front of a query block's window are never requested.  ``None``, ``(-1, -1)`` and, with ``is_causal=True``,
    ``(-1, 0)`` are the call without the keyword.  A bounded ``left`` needs ``is_causal=True``, ``right`` 0 or -1, ``causal_align="bottom_right"``,
    ``pv_accum_dtype="fp32+fp32"`` and the fused Q quantiser (``is_causal=False`` with a window is refused: the packed route has no operand for
    the diagonal's shift).  The pre-pass is the unwindowed call's: K mean, k scales and V scales over every key of a sequence.  Rows whose
    window holds no key give ``o = +0`` and ``lse = -inf``."""
    if pv_accum_dtype not in ("fp32", "fp32+fp32"):
        raise ValueError(f"Unsupported pv_accum_dtype: {pv_accum_dtype}")
    causal_align = kwargs.pop("causal_align", "top_left")
    if not isinstance(causal_align, str) or causal_align not in ("top_left", "bottom_right"):
        raise ValueError(f'causal_align must be "top_left" or "bottom_right" (got {causal_align!r})')
    bottom_right = causal_align == "bottom_right"
    # (the window first: what it needs is worded for its keyword)
    window = _varlen_window_args(kwargs.pop("window_size", None), is_causal, causal_align, pv_accum_dtype, max_seqlen_q, max_seqlen_k, kwargs)
    if bottom_right:
        if not is_causal:
            raise ValueError('causal_align="bottom_right" needs is_causal=True')
        if pv_accum_dtype != "fp32+fp32":
            raise ValueError(f'causal_align="bottom_right" needs pv_accum_dtype="fp32+fp32" (got {pv_accum_dtype!r})')
        if not kwargs.get("fuse_q_quant", True):
            raise ValueError('causal_align="bottom_right" needs the fused Q quantiser (fuse_q_quant=False is not supported)')
    st = _varlen_prepare(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal, sm_scale, smooth_k, kwargs, v_fp8=True,
                         bottom_right=bottom_right, window=window)
    o, lse = _varlen_attend_f8(st, pv_accum_dtype == "fp32+fp32", return_lse)
    if not return_lse:
        return o
    lse = lse / 1.44269504                 # kernel LSE: log2 units (core.py:328-329)
    if smooth_k:
        # q . km^T per (query head, packed row), km broadcast over the GQA group, in the input dtype as _lse_correction computes it
        # (the padded channels of km are zero: the unpadded q with the first head_dim channels of km gives the same products)
        Hq, Hkv = q.shape[1], st.km.shape[1]
        km = st.km[0, :, :q.shape[-1]]
        km = km if Hq == Hkv else torch.repeat_interleave(km, Hq // Hkv, dim=0)
        lse = lse + torch.matmul(q.transpose(0, 1), km.unsqueeze(-1)).squeeze(-1).to(torch.float32) * st.sm_scale
    return o, lse


_ROUTE_KWARGS = ("split_kv", "fused_prepass", "fuse_q_quant", "fp8_scores", "v_in_place", "split_kv_exact")


def _compiled_call(api, q, k, v, tensor_layout, is_causal, qk_quant_gran, sm_scale, pv_accum_dtype, smooth_k, smooth_v, return_lse,
                   kwargs=None):
    """torch.compile route of the dense CUDA-named entry points: one opaque custom op around the eager pipeline (ops.py).
    The op takes the default routes; a route override (``split_kv`` / ``fused_prepass`` / ``fuse_q_quant``) cannot travel through
    it, and a compiled run that silently took another route than the eager one would be a trap, so it is refused."""
    # (split_kv_exact=False is the default route: only a truthy flag is an override)
    given = [n for n in _ROUTE_KWARGS if kwargs and kwargs.get(n) is not None and (n != "split_kv_exact" or kwargs[n])]
    if given:
        raise ValueError(f"{', '.join(given)}: route overrides are not supported under torch.compile (the compiled op takes the default routes)")
    o, lse = ops.sageattn_call(q, k, v, api, tensor_layout, bool(is_causal), qk_quant_gran,
                               None if sm_scale is None else float(sm_scale), pv_accum_dtype, bool(smooth_k), bool(smooth_v),
                               bool(return_lse))
    return (o, lse) if return_lse else o


def _sm_log2(sm_scale: float) -> float:
    """sm_scale * log2(e) as the CUDA kernels form it: the Python double becomes a float kernel argument and is
    multiplied by the fp32 constant in fp32 (`sm_scale *= math::log2e`, qk_int_sv_f8_cuda_sm89.cuh:90, math.cuh:32).
    The product of two fp32 numbers is exact in a double, so one rounding to c_float is the fp32 product."""
    return ctypes.c_float(ctypes.c_float(sm_scale).value * ctypes.c_float(1.44269504088896340736).value).value


def _quant_q(q, qk_quant_gran, tensor_layout, warpq, sm_scale, blkk=64):
    """INT8 Q for the CUDA-named entry points.  Returns (q_int8, q_scale, gran code, q_warp, sm_scale_log2).  ``warpq``
    (32 / 16) and ``blkk`` (64 / 128) are the reference kernels' scale-group sizes (core.py:602-604, 964-970); the
    row -> group maps do not depend on the q block size, so BLKQ = 128 here also reproduces the sm90 kernels' BLKQ = 64 groups."""
    kflag = _cabi.GRAN_KBLK128 if blkk == 128 else 0
    if qk_quant_gran == "per_warp":            # quant.py:105-180 (q half)
        q_int8, q_scale = _quant(q, None, 128, warpq, _cabi.GRAN_PER_WARP, False, _cabi.QSTYLE_CUDA, 1.0, tensor_layout, 128 // warpq)
        return q_int8, q_scale, _cabi.GRAN_PER_WARP | kflag, warpq, _sm_log2(sm_scale)
    if qk_quant_gran == "per_thread":          # quant_per_thread.py:154-203 (q half)
        q_int8, q_scale = _quant(q, None, 128, warpq, _cabi.GRAN_PER_THREAD, False, _cabi.QSTYLE_TRITON_THREAD, 1.0, tensor_layout,
                                 (128 // warpq) * 8)
        return q_int8, q_scale, _cabi.GRAN_PER_THREAD | kflag, warpq, _sm_log2(sm_scale)
    if blkk != 64:
        raise ValueError("per_block scales are defined for 64-key groups only")
    # "per_block": gfx950 extension (the Triton path's granularity with the CUDA rounding); sm_scale * log2e folded into q
    q_int8, q_scale = _quant(q, None, 128, 128, _cabi.GRAN_PER_BLOCK, False, _cabi.QSTYLE_CUDA, sm_scale * LOG2E, tensor_layout, 1)
    return q_int8, q_scale, _cabi.GRAN_PER_BLOCK, 128, 1.0


def _fused_prepass_wanted(k, tensor_layout: str, override: Optional[bool]) -> bool:
    """Whether the K / V pre-pass runs as the one-launch, single-read kernel (``sage_prepass_kv``) or as the
    mean -> quantise -> statistics -> image sequence.  Same bits either way.  Measured on MI355X
    (profiles/r2_run_r3g_prepass_sweep.txt): the one launch wins from 512 keys up (129 vs 151 us at B=2 H=32 N=8192 D=128, 77 vs
    108 us at H=8 N=32768, 2x on launch-bound small calls) and loses only when very many heads of <= 256 keys leave its
    512-row slabs half empty (57 vs 47 us at B=64 H=16 N=256 D=64)."""
    if not prepass_fused_ok(k, tensor_layout):
        return False
    if override is not None:
        return bool(override)
    env = os.environ.get("SAGE_PREPASS", "")      # "seq" / "fused": force a route for every call (debugging, CU-masked streams)
    if env in ("seq", "sequence", "0"):
        return False
    if env in ("fused", "1"):
        return True
    B, H, L = _dims(k, tensor_layout)[:3]
    if L > 32768:
        # heads of 65 .. 128 slabs are within the barrier's reach (sage_prepass_max_seqlen = 65536) but every workgroup then waits for
        # 128 others: 325 vs 311 us at B=1 H=16 N=65536 (profiles/r3_run_f_prepass_64k.txt) -- the sequence unless the caller insists
        return False
    return L > 256 or B * H <= 256


def _prepass_kv(q, k, v, tensor_layout, qk_quant_gran, blkk, smooth_k, smooth_v, return_lse, fused: bool, v_fp8: bool = True,
                v_fp16: bool = False, kv_lens=None):
    """K mean + INT8 K (+ FP8 V image when ``v_fp8``).  Returns (lse_correction, km [B,H,D] | None, k_int8, k_scale, v_image,
    v_scale, vm); the K conventions are those of ``per_thread_int8`` / ``per_warp_int8`` / ``per_block_int8(cuda)``.
    ``kv_lens`` (int32 [B] on the device; per-thread groups, FP8 V, no ``smooth_v``): every statistic of sample b over its first
    ``kv_lens[b]`` rows only -- the kernel sequence whatever ``fused`` says (the one-launch pre-pass takes no lengths)."""
    if kv_lens is not None:
        assert qk_quant_gran == "per_thread" and blkk == 64 and v_fp8 and not smooth_v and not v_fp16
        km_s = channel_mean_kvlens(k, kv_lens, tensor_layout) if smooth_k else None
        lse_correction = None
        if smooth_k and return_lse:
            lse_correction = _lse_correction(q, km_s.unsqueeze(1 if tensor_layout == "NHD" else 2), tensor_layout)
        k_int8, k_scale = per_thread_int8_k_kvlens(k, km_s, kv_lens, tensor_layout)
        v_image, v_scale = per_channel_fp8_kvlens(v, kv_lens, tensor_layout, scale_max=448.0)
        return lse_correction, km_s, k_int8, k_scale, v_image, v_scale, None
    if fused:
        km_s, k_int8, k_scale, v_image, v_scale, vm = prepass_kv_fp8(k, v if (v_fp8 or v_fp16) else None, tensor_layout, smooth_k=smooth_k,
                                                                     smooth_v=smooth_v, BLKK=blkk, qk_quant_gran=qk_quant_gran, v_fp16=v_fp16)
        lse_correction = None
        if smooth_k and return_lse:
            lse_correction = _lse_correction(q, km_s.unsqueeze(1 if tensor_layout == "NHD" else 2), tensor_layout)
        return lse_correction, km_s, k_int8, k_scale, v_image, v_scale, vm
    km, lse_correction = _smooth_k(q, k, tensor_layout, smooth_k, return_lse)
    km_s = _squeeze_km(km, tensor_layout)
    if qk_quant_gran == "per_thread":
        k_int8, k_scale = _quant(k, km_s, blkk, blkk, _cabi.GRAN_PER_THREAD, True, _cabi.QSTYLE_TRITON_THREAD, 1.0, tensor_layout, 4)
    else:
        k_int8, k_scale = _quant(k, km_s, blkk, blkk, _cabi.GRAN_PER_BLOCK, True, _cabi.QSTYLE_CUDA, 1.0, tensor_layout, 1)
    v_image = v_scale = vm = None
    if v_fp8:
        v_image, v_scale, vm = per_channel_fp8(v, tensor_layout=tensor_layout, scale_max=448.0, smooth_v=smooth_v)
    return lse_correction, km_s, k_int8, k_scale, v_image, v_scale, vm


def sageattn_qk_int8_pv_fp16_cuda(q, k, v, tensor_layout: str = "HND", is_causal: bool = False,
                                  qk_quant_gran: str = "per_thread", sm_scale: Optional[float] = None,
                                  pv_accum_dtype: str = "fp32", smooth_k: bool = True, smooth_v: bool = False,
                                  return_lse: bool = False, **kwargs: Any):
    """INT8 QK^T + FP16 PV (reference core.py:451-633).  All three ``pv_accum_dtype`` values run the same arithmetic here: P.V is
    accumulated in FP32 (CDNA4's FP16 MFMA has no FP16 accumulator, so the reference's FP16 accumulator and its FP16 tile buffer
    have no counterpart) and the softmax denominator sums the fp16-ROUNDED probabilities in FP32, as the reference's tensor-core row
    sum does in every instantiation (qk_int_sv_f16_cuda_sm80.cu:313-320).  "fp16+fp32" differs from "fp32" only in the q scale groups
    the reference pairs with it (WARPQ = 16 at head_dim 128, core.py:602-604); "fp16" additionally honours ``smooth_v``."""
    if torch.compiler.is_compiling():
        return _compiled_call("fp16", q, k, v, tensor_layout, is_causal, qk_quant_gran, sm_scale, pv_accum_dtype, smooth_k, smooth_v, return_lse, kwargs)
    dtype = q.dtype
    _check_inputs(q, k, v)
    _check_shapes(q, k, v, tensor_layout)
    assert qk_quant_gran in ["per_warp", "per_thread", "per_block"], "qk_quant_gran must be either 'per_warp' or 'per_thread'."
    if pv_accum_dtype not in ("fp32", "fp16", "fp16+fp32"):
        raise ValueError(f"Unsupported pv_accum_dtype: {pv_accum_dtype}")
    torch.cuda.set_device(v.device)
    q, k, v, head_dim_og = _pad_head_dim(q, k, v)
    assert q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1, "Last dim of qkv must be contiguous."
    if sm_scale is None:
        sm_scale = head_dim_og ** -0.5
    if pv_accum_dtype in ["fp32", "fp16+fp32"] and smooth_v:
        warnings.warn(f"pv_accum_dtype is {pv_accum_dtype}, smooth_v will be ignored.")   # core.py:608-610
        smooth_v = False
    warpq = 16 if (q.size(-1) == 128 and pv_accum_dtype == "fp16+fp32") else 32              # core.py:602-604
    fused = _fused_prepass_wanted(k, tensor_layout, kwargs.get("fused_prepass"))
    # default route: Q is quantised inside the attention kernel (same bits, no INT8 copy of Q in HBM, one launch less)
    fuse_q = qk_quant_gran == "per_thread" and pv_accum_dtype != "fp16+fp32" and kwargs.get("fuse_q_quant", _FUSE_Q16_DEFAULT)
    n_split = 0
    if fuse_q:
        B_, Hq_, Lq_, _, _, _, _ = _dims(q, tensor_layout)
        n_split = _split_kv_plan(B_, Hq_, Lq_, _dims(k, tensor_layout)[2], is_causal, kwargs.get("split_kv"))
    # fp16 inputs on that route: the kernel reads V's rows in place, no V image and no V half of the pre-pass (core.py:613's
    # `v.to(torch.float16)` is the identity for them); same bits as the image route
    v_rows = fuse_q and not n_split and not smooth_v and _v_rows_wanted(q, k, v, tensor_layout, is_causal, kwargs.get("v_in_place"))
    v_in_prepass = fused and not smooth_v and not v_rows          # the fp16 image comes out of the same launch as K
    lse_correction, _, k_int8, k_scale, v_image, _, _ = _prepass_kv(q, k, v, tensor_layout, qk_quant_gran, 64, smooth_k, False, return_lse,
                                                                    fused, v_fp8=False, v_fp16=v_in_prepass)
    vm = None
    if smooth_v:     # pv_accum_dtype == "fp16": sub_mean + fused v_mean epilogue (core.py:617-619)
        v_image, vm = sub_mean(v, tensor_layout)
        vm = vm.float()
    elif not v_in_prepass and not v_rows:
        v_image = prep_v_fp16(v, tensor_layout)
    if fuse_q:
        if n_split:
            o, lse = _attn_fused_q_split(_aligned(q, 8), k_int8, v_image, None, k_scale, tensor_layout, is_causal, _sm_log2(sm_scale),
                                         n_split, return_lse, v_mean=vm)
        else:
            o, lse = _attn_fused_q(_aligned(q, 8), k_int8, v if v_rows else v_image, None, k_scale, tensor_layout, is_causal, _sm_log2(sm_scale),
                                   return_lse, v_mean=vm, v_rows=v_rows)
        return _finish(o, lse, head_dim_og, return_lse, smooth_k, lse_correction, sm_scale)
    q_int8, q_scale, gran, q_warp, sm_log2 = _quant_q(q, qk_quant_gran, tensor_layout, warpq, sm_scale)
    o, lse = _attn_dense(False, q_int8, k_int8, v_image, None, q_scale, k_scale, dtype, tensor_layout, is_causal,
                         gran, q_warp, sm_log2, pv_accum_dtype == "fp16+fp32", return_lse, v_mean=vm)
    return _finish(o, lse, head_dim_og, return_lse, smooth_k, lse_correction, sm_scale)


def sageattn_qk_int8_pv_fp8_cuda(q, k, v, tensor_layout: str = "HND", is_causal: bool = False,
                                 qk_quant_gran: str = "per_thread", sm_scale: Optional[float] = None,
                                 pv_accum_dtype: str = "fp32+fp16", smooth_k: bool = True, smooth_v: bool = False,
                                 return_lse: bool = False, kv_lens: Optional[torch.Tensor] = None, q_start=None,
                                 causal_align: str = "top_left", window_size=None, pack_gqa=None, num_splits=None, **kwargs: Any):
    """INT8 QK^T + FP8 (e4m3) PV (reference core.py:636-826).  "fp32+fp32" and "fp32+fp16" both
    run the two-level kernel with an FP32 tile buffer (gfx950's FP8 MFMA only writes FP32, so V
    keeps the full ``scale_max=448``; the reference's 2.25 is an FP16-accumulator artefact,
    core.py:805-807); "fp32" accumulates every tile straight into the output registers.

    ``split_kv_exact=True`` (gfx950 extension, opt-in): calls whose grid would not fill the chip -- few query rows against a long key range --
    run as key-range chunks whose running maximum starts at the unsplit call's, so every P is the unsplit call's and only the FP32 summation
    order of O and l differs (``split_kv``: None / "auto" plans S for non-causal calls, an integer S splits so, 0 never; a ragged rest of the
    key range runs as a tail chunk).  It needs the default path: per-thread granularity with the fused Q quantiser, two-level accumulation,
    the exact score form; anything else raises ValueError.

    ``kv_lens`` (gfx950 extension): an int32 / int64 tensor ``[B]`` on q's device for a dense, right-padded batch -- sample b attends to keys
    ``0 .. kv_lens[b] - 1`` of ``k[b]`` / ``v[b]`` and to nothing else (causal: ``key <= row and key < kv_lens[b]``, top-left aligned).  Its
    ``o`` and ``lse`` are, bit for bit, what this function returns for ``(q[b:b+1], k[b:b+1, :, :len_b], v[b:b+1, :, :len_b])``: the K mean,
    the K scale groups and the V scales are formed over the valid rows only, and the padding rows are never read (they may be
    uninitialised).  The lengths are clamped to ``[0, kv_len]`` on the device and never read by the host, so the call can be captured in a
    HIP graph and replayed with other lengths in the same tensor; ``kv_lens[b] == 0`` gives ``o[b] = 0`` and ``lse[b] = -inf``.  The default
    path only: per-thread granularity with the fused Q quantiser, two-level accumulation, the exact score form, no ``smooth_v``, no
    split-KV, not under torch.compile; anything else raises ValueError.

    ``q_start`` / ``causal_align`` (gfx950 extension, ``is_causal=True`` only): where the causal diagonal of each sample lies.  ``q_start[b]``
    -- an int32 / int64 tensor ``[B]`` on q's device, or a Python int for the whole batch -- is the position of query row 0 of sample b on
    the key axis: row i attends to key j iff ``j <= q_start[b] + i`` and ``j < len_b``, ``len_b = clamp(kv_lens[b], 0, kv_len)`` (``kv_len``
    without ``kv_lens``).  ``q_start == 0`` is the top-left mask above; ``q_start[b] = len_b - qo_len`` is the bottom-right one (torch's
    ``causal_lower_right``, FlashAttention >= 2.1), what a caller who continues a sequence needs -- chunked prefill, speculative-decode
    verification, a prompt continued against a cached prefix: ``qo_len`` new rows against ``len_b`` cached-plus-new keys.
    ``causal_align="bottom_right"`` is that choice spelled out: ``clamp(kv_lens, 0, kv_len) - qo_len`` formed on the device, the constant
    ``kv_len - qo_len`` without ``kv_lens``; giving both keywords raises ValueError.  The offsets are clamped to ``[-qo_len, kv_len]`` on the
    device and never read by the host: no synchronisation, grids and allocations follow from the shapes, the call captures into a HIP graph
    and a replay computes with what ``q_start`` / ``kv_lens`` hold then.  A row with ``q_start[b] + i < 0``, and every row of a sample with
    ``len_b == 0``, sees nothing: ``o = +0``, ``lse = -inf``, never NaN.  Key rows from ``len_b`` on are never read.  Offsets that are
    multiples of 64 keep the pipelined diagonal tiles; any other offset runs the diagonal of each 128-row query block as three general
    tiles -- correct, slower.  The route is ``kv_lens``'s (without ``kv_lens`` the attention entry gets lengths filled with
    ``kv_len`` and the plain pre-pass runs, the one-launch route included), so its restrictions hold and raise ValueError: per-thread
    granularity with the fused Q quantiser, two-level accumulation, the exact score form, no ``smooth_v``, no split-KV (a decode-shaped
    call of ``qo_len <= 128`` therefore launches ``B * Hq`` workgroups), not under torch.compile.

    ``window_size=(left, right)`` (gfx950 extension; FlashAttention's convention: ints, ``-1`` = unbounded on that side, ``None`` or
    ``(-1, -1)`` = no window): a bounded look-back without a mask tensor.  With the sample's offset ``s_b`` (``q_start[b]``, or what
    ``causal_align`` forms, default 0), a window of ``W`` keys and a diagonal shift ``r``, row i attends to key j iff
    ``s_b + r + i - W < j <= s_b + r + i`` and ``0 <= j < len_b``.  ``is_causal=True``: ``right`` must be 0 or -1, ``W = left + 1``, ``r = 0``.
    ``is_causal=False`` with ``right >= 0``: the call runs the causal kernels with the diagonal moved right, ``r = right`` (added to the offsets
    on the device, no host read) and ``W = left + right + 1``, unbounded for ``left = -1``; ``q_start`` is accepted here as the rows' position
    on the key axis.  The window is a Python int, a property of the model and a constant of a captured graph.  A work item starts at the
    64-key tile of the first key its rows see and ends at its diagonal: tiles outside are never requested, and key rows, k scales and V
    images in front of the first one are never read.  The K mean, the K scale groups and the V scales are those of the call without the
    window on the same ``kv_lens`` (the window masks scores, it does not change operands).  A row whose window holds no key -- in front of
    key 0, or wholly behind ``len_b`` -- gives ``o = +0``, ``lse = -inf``.  A window that cuts no row (``left >= kv_len + qo_len``) gives
    the bits of the call without it.  The restrictions are ``q_start``'s and raise ValueError naming ``window_size``.

    ``pack_gqa`` (gfx950 extension; ``None`` / ``False``: today's launch): ``True`` packs the query heads of a GQA group into one workgroup for
    a decode-shaped call, ``qo_len <= 32`` and ``num_qo_heads / num_kv_heads >= 2``.  The kernel's work item is 128 query rows of one query
    head, 32 per wave: with at most 32 rows three of four waves hold none and still run every tile, and each query head of a group streams
    the same K tiles and V images.  Packed, a workgroup serves four query heads of one kv head, one wave each, over one shared K / V ring:
    ``B * Hkv * ceil(group / 4)`` workgroups instead of ``B * Hq``.  ``o`` and ``lse`` are, bit for bit, those of the same call with
    ``pack_gqa=False`` -- on every input, and nothing else is promised.  It combines with ``kv_lens``, ``q_start`` / ``causal_align`` and
    ``window_size`` in every combination they take; alone, the call takes the ``kv_lens`` attention entry with lengths filled with ``kv_len``
    behind the plain pre-pass.  The route's restrictions are ``kv_lens``'s and raise ValueError naming ``pack_gqa``, as do ``qo_len > 32``,
    ``num_qo_heads == num_kv_heads`` and use under torch.compile.

    ``num_splits`` (gfx950 extension; ``None`` / ``1``: today's call, every bit, launch and grid unchanged): an int ``2 .. 255`` runs a call
    of one query block (``qo_len <= 128``) as that many key-range chunks, so that few sequences with long key ranges fill the device:
    ``B * Hq * S`` workgroups, ``B * Hkv * ceil(group / 4) * S`` with ``pack_gqa=True``.  It is exact: a first launch computes each chunk's
    row maxima with the attention kernel's arithmetic, each chunk then starts its running maximum where the unsplit call's stands at the
    chunk's first tile, and an FP32 merge adds the chunks up -- every P is the P of the call without ``num_splits``, only the FP32 summation
    order of O and l differs.  ``T = ceil(ceil(kv_len / 64) / S)`` tiles per chunk from the padded ``kv_len``; chunk c of sample b holds keys
    ``[64 T c, 64 T (c + 1))`` below ``len_b``, the causal limit in global key coordinates: no divisibility rule, and a chunk that holds no
    visible key -- past ``len_b``, behind the diagonal, of an empty sample -- requests no tile and weighs nothing.  ``"auto"`` / ``0`` plans
    S from the shapes alone and splits only inside the region a probe measured the route faster in: at most 64 unsplit workgroups, 8192 to
    65536 keys, at most 32 query rows.  The keyword rides on
    the ``kv_lens`` family as ``pack_gqa`` does and combines with ``kv_lens``, ``q_start``, ``causal_align="bottom_right"`` and
    ``pack_gqa=True`` (whose own rules hold); without ``kv_lens`` the lengths are filled with ``kv_len`` on the device, and ``is_causal=True``
    without offsets is the top-left mask.  The workspace is allocated from the shapes, nothing reads lengths or offsets on the host: the call
    captures into a HIP graph and a replay follows the length tensor's contents.  The route's restrictions are ``kv_lens``'s and raise
    ValueError naming ``num_splits``, as do ``qo_len > 128``, a ``window_size`` that bounds the look-back, a value that is no int in
    ``[0, 255]`` nor ``"auto"`` and use under torch.compile."""
    if torch.compiler.is_compiling():
        _refuse_kv_family_compiled(kv_lens, q_start, causal_align, window_size, pack_gqa, num_splits, " (the compiled op takes the default routes)")
        return _compiled_call("fp8", q, k, v, tensor_layout, is_causal, qk_quant_gran, sm_scale, pv_accum_dtype, smooth_k, smooth_v, return_lse, kwargs)
    _check_shapes(q, k, v, tensor_layout)
    call = _kv_family_args(q, k, tensor_layout, is_causal, kv_lens, q_start, causal_align, window_size, pack_gqa, num_splits,
                           qk_quant_gran, pv_accum_dtype, smooth_v, kwargs)
    exact = _split_exact_args(kwargs, qk_quant_gran, pv_accum_dtype, _dims(k, tensor_layout)[2])
    dtype = q.dtype
    _check_inputs(q, k, v)
    assert qk_quant_gran in ["per_warp", "per_thread", "per_block"], "qk_quant_gran must be either 'per_warp' or 'per_thread'."
    if pv_accum_dtype not in ("fp32", "fp32+fp32", "fp32+fp16"):
        raise ValueError(f"Unsupported pv_accum_dtype: {pv_accum_dtype}")
    torch.cuda.set_device(v.device)
    q, k, v, head_dim_og = _pad_head_dim(q, k, v)
    assert q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1, "Last dim of qkv must be contiguous."
    if sm_scale is None:
        sm_scale = head_dim_og ** -0.5
    if pv_accum_dtype in ("fp32+fp32", "fp32+fp16") and smooth_v:
        warnings.warn(f"pv_accum_dtype is '{pv_accum_dtype}', smooth_v will be ignored.")   # core.py:797-803
        smooth_v = False
    fuse_q = qk_quant_gran == "per_thread" and pv_accum_dtype != "fp32" and kwargs.get("fuse_q_quant", True)
    fused = _fused_prepass_wanted(k, tensor_layout, kwargs.get("fused_prepass"))
    folded = ops.fp8_folded(kwargs.get("fp8_scores"))
    if call.with_lens or call.with_start or call.gqa_pack or call.splits:
        # the kv_lens attention entry (under a window the call is causal: call.is_causal).  With kv_lens: the length-aware kernel sequence (mean ->
        # K quantiser -> V statistics -> V image), never the one-launch pre-pass; int64 lengths are converted on the device.  Without (offsets,
        # packed GQA groups, key-range chunks alone): the plain pre-pass and lengths filled with kv_len -- full lengths give the plain call's
        # bits; is_causal without offsets is the top-left mask (the split's causal kernels take offsets, and none means 0).
        if call.with_lens:
            lens = kv_lens.to(torch.int32).contiguous()
            prepass = dict(fused=False, kv_lens=lens)
        else:
            lens = torch.full((_dims(q, tensor_layout)[0],), _dims(k, tensor_layout)[2], dtype=torch.int32, device=q.device)
            prepass = dict(fused=fused)
        lse_correction, _, k_int8, k_scale, v_image, v_scale, _ = _prepass_kv(q, k, v, tensor_layout, "per_thread", 64, smooth_k, False, return_lse,
                                                                              **prepass)
        return _attn_kv_family(call, q, lens, kv_lens, k_int8, v_image, v_scale, k_scale, tensor_layout, sm_scale, return_lse, head_dim_og,
                               smooth_k, lse_correction)
    if fuse_q:
        # default route: Q is quantised inside the attention kernel (same bits, no INT8 copy of Q in HBM).
        # (Running the V pre-pass on a side stream beside the K chain was measured and rejected: the two HBM-bound chains
        #  slow each other down and the cross-stream joins cost more than the launch gaps they hide, 956 -> 1130 us at C3.)
        lse_correction, _, k_int8, k_scale, v_image, v_scale, vm = _prepass_kv(q, k, v, tensor_layout, "per_thread", 64, smooth_k, smooth_v,
                                                                               return_lse, fused)
        B_, Hq_, Lq_, _, _, _, _ = _dims(q, tensor_layout)
        if exact:
            n_split = _split_exact_plan(B_, Hq_, Lq_, _dims(k, tensor_layout)[2], is_causal, kwargs.get("split_kv"))
            if n_split:
                o, lse = _attn_fused_q_split_exact(_aligned(q, 8), k_int8, v_image, v_scale, k_scale, tensor_layout, is_causal,
                                                   _sm_log2(sm_scale), n_split, return_lse, v_mean=vm)
                return _finish(o, lse, head_dim_og, return_lse, smooth_k, lse_correction, sm_scale)
        else:
            n_split = _split_kv_plan(B_, Hq_, Lq_, _dims(k, tensor_layout)[2], is_causal, kwargs.get("split_kv"), auto_default=False)
        if n_split:
            o, lse = _attn_fused_q_split(_aligned(q, 8), k_int8, v_image, v_scale, k_scale, tensor_layout, is_causal,
                                         _sm_log2(sm_scale), n_split, return_lse, v_mean=vm, folded_scores=folded)
        else:
            o, lse = _attn_fused_q(_aligned(q, 8), k_int8, v_image, v_scale, k_scale, tensor_layout, is_causal, _sm_log2(sm_scale),
                                   return_lse, v_mean=vm, folded_scores=folded)
        return _finish(o, lse, head_dim_og, return_lse, smooth_k, lse_correction, sm_scale)
    lse_correction, _, k_int8, k_scale, v_image, v_scale, vm = _prepass_kv(q, k, v, tensor_layout, qk_quant_gran, 64, smooth_k, smooth_v,
                                                                           return_lse, fused)
    q_int8, q_scale, gran, q_warp, sm_log2 = _quant_q(q, qk_quant_gran, tensor_layout, 32, sm_scale)
    o, lse = _attn_dense(True, q_int8, k_int8, v_image, v_scale, q_scale, k_scale, dtype, tensor_layout, is_causal,
                         gran, q_warp, sm_log2, pv_accum_dtype != "fp32", return_lse, v_mean=vm, folded_scores=folded)
    return _finish(o, lse, head_dim_og, return_lse, smooth_k, lse_correction, sm_scale)


def sageattn_qk_int8_pv_fp8_cuda_sm90(q, k, v, tensor_layout: str = "HND", is_causal: bool = False,
                                      qk_quant_gran: str = "per_thread", sm_scale: Optional[float] = None,
                                      pv_accum_dtype: str = "fp32+fp32", smooth_k: bool = True, return_lse: bool = False,
                                      **kwargs: Any):
    """Kept for drop-in (reference core.py:829-996).  Same gfx950 kernel and two-level accumulation as
    ``sageattn_qk_int8_pv_fp8_cuda``, with the sm90 kernels' scale groups: q per 16 rows (per-warp) or the 8 per-thread
    slots of every 16 rows, k per 128 keys (core.py:964-970: BLKQ=64, WARPQ=16, BLKK=128, WARPK=128)."""
    if pv_accum_dtype == "fp32":
        raise NotImplementedError("Please use pv_accum_dtype='fp32+fp32' for sm90.")   # core.py:985-986
    if pv_accum_dtype != "fp32+fp32":
        raise ValueError(f"Unsupported pv_accum_dtype: {pv_accum_dtype}")
    if torch.compiler.is_compiling():
        return _compiled_call("sm90", q, k, v, tensor_layout, is_causal, qk_quant_gran, sm_scale, pv_accum_dtype, smooth_k, False, return_lse, kwargs)
    dtype = q.dtype
    _check_inputs(q, k, v)
    _check_shapes(q, k, v, tensor_layout)
    assert qk_quant_gran in ["per_warp", "per_thread"], "qk_quant_gran must be either 'per_warp' or 'per_thread'."
    torch.cuda.set_device(v.device)
    q, k, v, head_dim_og = _pad_head_dim(q, k, v)
    assert q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1, "Last dim of qkv must be contiguous."
    if sm_scale is None:
        sm_scale = head_dim_og ** -0.5
    fused = _fused_prepass_wanted(k, tensor_layout, kwargs.get("fused_prepass"))
    lse_correction, _, k_int8, k_scale, v_image, v_scale, _ = _prepass_kv(q, k, v, tensor_layout, qk_quant_gran, 128, smooth_k, False,
                                                                          return_lse, fused)
    q_int8, q_scale, gran, q_warp, sm_log2 = _quant_q(q, qk_quant_gran, tensor_layout, 16, sm_scale, blkk=128)
    o, lse = _attn_dense(True, q_int8, k_int8, v_image, v_scale, q_scale, k_scale, dtype, tensor_layout, is_causal,
                         gran, q_warp, sm_log2, True, return_lse, folded_scores=ops.fp8_folded(kwargs.get("fp8_scores")))
    return _finish(o, lse, head_dim_og, return_lse, smooth_k, lse_correction, sm_scale)
