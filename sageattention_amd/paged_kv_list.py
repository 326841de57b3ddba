"""The step call on the paged quantised KV cache over device-built work lists, heaviest first (gfx950 extension).

:func:`~sageattention_amd.paged_kv_step.sageattn_kvcache_step` deals each of its two launches to the eight XCDs as one contiguous run of the
dense grid: the chunk sequences of a step -- or its long decode contexts -- that sit in adjacent slots are one XCD's work.
:func:`sageattn_kvcache_step_listed` takes the same operands and puts one small launch in front that sorts the step on the device: the decode
sequences by their context, every 128-row block of the chunk sequences by the key tiles it visits.  The two attention launches then take their
items from those lists, round-robin over the XCDs.  Three launches (two when ``max_seqlen_q <= 32``), no host read; every row is bit for bit
what ``sageattn_kvcache_step`` returns (``sage_kvlist_attn``, include/sage_kvlist_gfx950.h).

Import from here; the name is not part of the package's ``__all__`` and the call is a default of nothing.  Not under torch.compile.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _cabi, _cabi_kvlist, core, ops
from .paged_kv_varlen import _host_max, _packed, _paged, _prefix
from .quant import _aligned, _dtype_code, _p, _stream

__all__ = ["sageattn_kvcache_step_listed"]


@torch.compiler.disable
def sageattn_kvcache_step_listed(q: torch.Tensor, cache, cu_seqlens_q: torch.Tensor, max_seqlen_q: int, q_start=None, window_size=None,
                                 sm_scale: Optional[float] = None, return_lse: bool = False, return_plan: bool = False):
    """:func:`~sageattention_amd.paged_kv_step.sageattn_kvcache_step` with its launches over work lists: every argument means what it means
    there, and so do the results, bit for bit.  ``return_plan=True`` adds the workspace as the last result: an int32 tensor holding
    ``hdr[16]`` = ``{n_decode, n_chunk_items, group, fold, left, ...}``, ``decode_list[B]`` and the ``(sequence, query block)`` pairs of the chunk
    list (include/sage_kvlist_gfx950.h); entries past the two counts are not written.

    The decode launch has ``8 * ceil(B * Hkv / 8) * ceil(group / 4)`` workgroups, the chunk launch -- only when ``max_seqlen_q > 32`` -- those of a
    dense launch over ``Hq`` heads of ``min(B * ceil(max_seqlen_q / 128), total // 128 + min(B, total // 33))`` items; a workgroup past a list's
    count leaves at once.  The call captures into a HIP graph; a replay sorts by the contents of the arrays.

    ValueError as ``sageattn_kvcache_step`` raises them, and for more sequences than one plan launch takes (``sage_varlen_plan_max_seqs()``)."""
    name = "sageattn_kvcache_step_listed"
    if torch.compiler.is_compiling():
        raise ValueError(f"{name} is not supported under torch.compile")
    _paged(name, cache)
    _packed("q", q, None, cache)
    total, Hq, D = q.shape
    if Hq % cache.Hkv != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by the cache's num_kv_heads ({cache.Hkv})")
    if Hq // cache.Hkv < 2:
        raise ValueError(f"{name} packs the query heads of a GQA group: Hq / Hkv must be at least 2 (got {Hq} / {cache.Hkv}); "
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
    lib = _cabi_kvlist.load()
    if B > _cabi.load().sage_varlen_plan_max_seqs():
        raise ValueError(f"{name} takes at most {_cabi.load().sage_varlen_plan_max_seqs()} sequences, the ones a plan launch sorts (got {B})")
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
    ws_bytes = lib.sage_kvlist_ws_bytes(B, total, max_seqlen_q)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=q.device)
    attr = _cabi.launch_attr(grid_out=ops._hooks.grid_probe, q_start=start, window=call.window)
    code = _dtype_code(q)
    rc = lib.sage_kvlist_attn(
        _p(q), _p(cache.k_int8), _p(cache.v_image), _p(o), _p(lse), _p(cache.k_scale), _p(cache.v_scale), _p(cache.lens), _p(cu),
        _p(cache.block_table), cache.block_table.stride(0), cache.num_pages, cache.page_size, cache.max_pages_per_seq,
        B, Hq, cache.Hkv, total, max_seqlen_q, D, q.stride(0), q.stride(1),
        cache.k_int8.stride(0), cache.k_int8.stride(1), cache.k_int8.stride(2), o.stride(0), o.stride(1), total,
        1, core._sm_log2(sm_scale), code, code, _stream(q), _cabi.attr_arg(attr), _p(ws), ws_bytes)
    ops.attn_check(rc, "sage_kvlist_attn", attr, q.device)
    out = (o,)
    if return_lse:
        lse = lse / 1.44269504                 # kernel LSE: log2 units
        if cache.k_mean is not None:
            # q . km^T per (query head, packed row) with the mean of the row's own sequence, as sageattn_kvcache_step forms it
            seq = torch.bucketize(torch.arange(total, device=q.device, dtype=torch.int32), cu[1:], right=True).clamp(max=B - 1)
            km = cache.k_mean.index_select(0, seq)                                      # [total, Hkv, D]
            km = torch.repeat_interleave(km, Hq // cache.Hkv, dim=1)                    # [total, Hq, D]
            corr = torch.matmul(q.unsqueeze(2), km.unsqueeze(3)).reshape(total, Hq).to(torch.float32)
            lse = lse + corr.transpose(0, 1) * sm_scale
        out += (lse,)
    if return_plan:
        out += (ws,)
    return out[0] if len(out) == 1 else out
