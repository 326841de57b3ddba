"""One attention call per engine step on the paged quantised KV cache (gfx950 extension).

:func:`~sageattention_amd.paged_kv_varlen.sageattn_kvcache_varlen` runs every packed query row on the 128-row kernel, one workgroup per query
head: a decoding sequence's single row streams that sequence's K / V once per query head.  :func:`sageattn_kvcache_step` takes the same
operands and sorts the sequences on the device, by the row count their two ``cu_seqlens_q`` words give: a sequence of 1 .. 32 rows runs the
packed-group kernel of ``pack_gqa`` -- the query heads of a GQA group four to a workgroup over one K / V stream -- and a longer one the 128-row
kernel.  Two launches (one when ``max_seqlen_q <= 32``), no host read, no padding; every row is bit for bit what ``sageattn_kvcache_varlen``
returns (``sage_kvstep_attn``, include/sage_kvstep_gfx950.h).

Import from here; the name is not part of the package's ``__all__``.  Not under torch.compile.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _cabi, _cabi_kvstep, core, ops
from .paged_kv_varlen import _host_max, _packed, _paged, _prefix
from .quant import _aligned, _dtype_code, _p, _stream

__all__ = ["sageattn_kvcache_step"]


@torch.compiler.disable
def sageattn_kvcache_step(q: torch.Tensor, cache, cu_seqlens_q: torch.Tensor, max_seqlen_q: int, q_start=None, window_size=None,
                          sm_scale: Optional[float] = None, return_lse: bool = False):
    """:func:`~sageattention_amd.paged_kv_varlen.sageattn_kvcache_varlen` with the decode rows of a GQA group packed: every argument means what
    it means there, and so do the results -- ``o`` ``[total, Hq, D]``, with ``return_lse`` also ``lse`` fp32 ``[Hq, total]`` in natural-log
    units with each token's own sequence's K-mean correction, rows of a sequence beyond ``max_seqlen_q`` not computed, rows no sequence owns not
    written -- bit for bit.

    A sequence with 1 .. 32 rows (after the clamp to ``max_seqlen_q``: a longer one cut to at most 32 rows counts) costs ``Hkv * ceil(group / 4)``
    workgroups that stream its K / V once per four query heads; a longer one ``Hq * ceil(rows / 128)`` workgroups as before.  Each launch covers
    its whole grid -- ``B * Hkv * ceil(group / 4)`` workgroups, and ``B * Hq * ceil(max_seqlen_q / 128)`` more when ``max_seqlen_q > 32`` -- and a
    workgroup whose sequence belongs to the other launch leaves at once.  The call captures into a HIP graph; a replay sorts by the contents
    of ``cu_seqlens_q``.

    ValueError for a contiguous ``QuantizedKVCache``, an unseeded cache and ``Hq / Hkv < 2`` (no GQA group to pack: ``sageattn_kvcache_varlen``
    is the call)."""
    if torch.compiler.is_compiling():
        raise ValueError("sageattn_kvcache_step is not supported under torch.compile")
    _paged("sageattn_kvcache_step", cache)
    _packed("q", q, None, cache)
    total, Hq, D = q.shape
    if Hq % cache.Hkv != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by the cache's num_kv_heads ({cache.Hkv})")
    if Hq // cache.Hkv < 2:
        raise ValueError(f"sageattn_kvcache_step packs the query heads of a GQA group: Hq / Hkv must be at least 2 (got {Hq} / {cache.Hkv}); "
                         "sageattn_kvcache_varlen takes such a call")
    if q.stride(-1) != 1:
        raise ValueError("Last dim of q must be contiguous.")
    B = cache.B
    cu = _prefix("cu_seqlens_q", cu_seqlens_q, B, cache.device)
    max_seqlen_q = _host_max("max_seqlen_q", max_seqlen_q)
    # the keywords' checks and meanings are the kv_lens family's: one resolver, which reads shapes alone -- q's as the dense call's [B, Hq, Lq, D]
    q_shape = q.as_strided((B, Hq, max_seqlen_q, D), (0, 0, 0, 1))
    call = core._kv_family_args(q_shape, cache._k_logical("HND"), "HND", True, None, q_start, "bottom_right" if q_start is None else "top_left",
                                window_size, None, None, "per_thread", "fp32+fp16", False, {})
    torch.cuda.set_device(q.device)
    if sm_scale is None:
        sm_scale = D ** -0.5
    counts = (cu[1:] - cu[:-1]).to(torch.int64)
    if call.q_start is None:       # bottom-right: the sequence's last row at its last key
        start = (cache.lens.clamp(0, cache.capacity).to(torch.int64) - counts).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32)
    else:
        start = core._q_start_tensor(call.q_start, None, B, max_seqlen_q, cache.capacity, q.device, call.shift)
    q = _aligned(q, 8)
    o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    lse = torch.empty((Hq, total), dtype=torch.float32, device=q.device) if return_lse else None
    attr = _cabi.launch_attr(grid_out=ops._hooks.grid_probe, q_start=start, window=call.window)
    code = _dtype_code(q)
    rc = _cabi_kvstep.load().sage_kvstep_attn(
        _p(q), _p(cache.k_int8), _p(cache.v_image), _p(o), _p(lse), _p(cache.k_scale), _p(cache.v_scale), _p(cache.lens), _p(cu),
        _p(cache.block_table), cache.block_table.stride(0), cache.num_pages, cache.page_size, cache.max_pages_per_seq,
        B, Hq, cache.Hkv, total, max_seqlen_q, D, q.stride(0), q.stride(1),
        cache.k_int8.stride(0), cache.k_int8.stride(1), cache.k_int8.stride(2), o.stride(0), o.stride(1), total,
        1, core._sm_log2(sm_scale), code, code, _stream(q), _cabi.attr_arg(attr))
    ops.attn_check(rc, "sage_kvstep_attn", attr, q.device)
    if not return_lse:
        return o
    lse = lse / 1.44269504                 # kernel LSE: log2 units
    if cache.k_mean is not None:
        # q . km^T per (query head, packed row) with the mean of the row's own sequence, as sageattn_kvcache_varlen forms it
        seq = torch.bucketize(torch.arange(total, device=q.device, dtype=torch.int32), cu[1:], right=True).clamp(max=B - 1)
        km = cache.k_mean.index_select(0, seq)                                      # [total, Hkv, D]
        km = torch.repeat_interleave(km, Hq // cache.Hkv, dim=1)                    # [total, Hq, D]
        corr = torch.matmul(q.unsqueeze(2), km.unsqueeze(3)).reshape(total, Hq).to(torch.float32)
        lse = lse + corr.transpose(0, 1) * sm_scale
    return o, lse
