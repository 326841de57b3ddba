"""The listed step call on the paged quantised KV cache with its decode sequences split over the key range, exactly (gfx950 extension).

:func:`~sageattention_amd.paged_kv_list.sageattn_kvcache_step_listed` runs a decode sequence -- one of 1 .. 32 query rows -- as
``Hkv * ceil(group / 4)`` serial chains over its whole context, so a step of a handful of long contexts leaves most of the device idle;
:func:`~sageattention_amd.paged_kv_split.sageattn_kvcache_split` fills it, but takes dense queries.  :func:`sageattn_kvcache_step_split` is the
listed step call with every decode sequence run as ``num_splits`` key-range chunks: a plan launch, the chunk maxima, the seeded chunks with
FP32 partials, the merge, then the listed call's chunk launch for the longer sequences.  A decode sequence's rows are bit for bit what
``sageattn_kvcache_split(q_dense, cache, num_splits, is_causal=True, pack_gqa=True, ...)`` returns for that sample with a dense ``q`` of as many
rows; every other row is bit for bit ``sageattn_kvcache_step_listed``'s (``sage_kvlsplit_attn``, include/sage_kvlsplit_gfx950.h).

Import from here; the name is not part of the package's ``__all__`` and the call is a default of nothing.  Not under torch.compile.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _cabi, _cabi_kvlsplit, core, ops
from .paged_kv_list import sageattn_kvcache_step_listed
from .paged_kv_varlen import _host_max, _packed, _paged, _prefix
from .quant import _aligned, _dtype_code, _p, _stream

__all__ = ["sageattn_kvcache_step_split"]


def _splits(name: str, num_splits, B: int, Hq: int, Hkv: int, max_seqlen_q: int, capacity: int) -> int:
    """The chunk count ``num_splits`` asks for, 0 for the listed call itself: ``None`` / ``1`` are that call, ``"auto"`` / ``0`` the kv_lens
    family's plan (``core._num_splits_plan``) for packed decode rows on the logical capacity, an int in [2, 255] itself."""
    if num_splits is None:
        return 0
    auto = isinstance(num_splits, str) and num_splits == "auto"
    if isinstance(num_splits, bool) or not (auto or (isinstance(num_splits, int) and 0 <= num_splits <= 255)):
        raise ValueError(f"{name}: num_splits must be None, an int in [0, 255] or 'auto' (got {num_splits!r})")
    if auto or num_splits == 0:
        return core._num_splits_plan(B, Hq, Hkv, min(max_seqlen_q, 32), capacity, True)
    return 0 if num_splits == 1 else num_splits


@torch.compiler.disable
def sageattn_kvcache_step_split(q: torch.Tensor, cache, cu_seqlens_q: torch.Tensor, max_seqlen_q: int, num_splits, q_start=None,
                                sm_scale: Optional[float] = None, return_lse: bool = False):
    """:func:`~sageattention_amd.paged_kv_list.sageattn_kvcache_step_listed` with every decode sequence as ``num_splits`` key-range chunks.

    ``q`` ``[total, Hq, D]``, ``cache``, ``cu_seqlens_q``, ``max_seqlen_q``, ``q_start``, ``sm_scale`` and ``return_lse`` mean what they mean
    there; ``window_size`` is not offered.  ``num_splits``: an int in ``[2, 255]`` -- one host-known number per call, a chunk is
    ``ceil(ceil(capacity / 64) / num_splits)`` whole 64-key tiles of the logical key axis for every sequence, so a sequence shorter than the
    capacity has empty trailing chunks (an early exit and one word each); ``None`` / ``1``: the listed call itself, the same bits; ``"auto"`` /
    ``0``: ``core._num_splits_plan(B, Hq, Hkv, min(max_seqlen_q, 32), capacity, True)``, where 0 is the listed call.

    The split workspace -- ``min(max_seqlen_q, 32)`` rows per (sequence, head, chunk) -- is a ``torch.empty`` from the shapes.  No host read,
    no synchronisation: the call captures into a HIP graph.

    ValueError by name for a ``QuantizedKVCache``, an unseeded cache, ``Hq / Hkv < 2`` and a bad ``num_splits``, else as the listed call."""
    name = "sageattn_kvcache_step_split"
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
    B = cache.B
    mq = _host_max("max_seqlen_q", max_seqlen_q)
    S = _splits(name, num_splits, B, Hq, cache.Hkv, mq, cache.capacity)
    if S == 0:
        return sageattn_kvcache_step_listed(q, cache, cu_seqlens_q, max_seqlen_q, q_start=q_start, sm_scale=sm_scale, return_lse=return_lse)
    if q.stride(-1) != 1:
        raise ValueError("Last dim of q must be contiguous.")
    cu = _prefix("cu_seqlens_q", cu_seqlens_q, B, cache.device)
    max_seqlen_q = mq
    # the keywords' checks and meanings are the kv_lens family's: one resolver, which reads shapes alone -- q's as the dense call's [B, Hq, Lq, D]
    q_shape = q.as_strided((B, Hq, max_seqlen_q, D), (0, 0, 0, 1))
    call = core._kv_family_args(q_shape, cache._k_logical("HND"), "HND", True, None, q_start, "bottom_right" if q_start is None else "top_left",
                                None, None, None, "per_thread", "fp32+fp16", False, {})
    lib = _cabi_kvlsplit.load()
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
    list_bytes = lib.sage_kvlist_ws_bytes(B, total, max_seqlen_q)
    list_ws = torch.empty(list_bytes // 4, dtype=torch.int32, device=q.device)
    split_ws = torch.empty((_cabi.kv_split_ws_bytes(B, Hq, min(max_seqlen_q, 32), D, S) // 4,), dtype=torch.float32, device=q.device)
    attr = _cabi.launch_attr(launch_ws=split_ws, grid_out=ops._hooks.grid_probe, q_start=start, kv_split=S)
    code = _dtype_code(q)
    rc = lib.sage_kvlsplit_attn(
        _p(q), _p(cache.k_int8), _p(cache.v_image), _p(o), _p(lse), _p(cache.k_scale), _p(cache.v_scale), _p(cache.lens), _p(cu),
        _p(cache.block_table), cache.block_table.stride(0), cache.num_pages, cache.page_size, cache.max_pages_per_seq,
        B, Hq, cache.Hkv, total, max_seqlen_q, D, q.stride(0), q.stride(1),
        cache.k_int8.stride(0), cache.k_int8.stride(1), cache.k_int8.stride(2), o.stride(0), o.stride(1), total,
        1, core._sm_log2(sm_scale), code, code, _stream(q), _cabi.attr_arg(attr), _p(list_ws), list_bytes)
    ops.attn_check(rc, "sage_kvlsplit_attn", attr, q.device)
    if not return_lse:
        return o
    lse = lse / 1.44269504                 # kernel LSE: log2 units
    if cache.k_mean is not None:
        # q . km^T per (query head, packed row) with the mean of the row's own sequence, as sageattn_kvcache_step_listed forms it
        seq = torch.bucketize(torch.arange(total, device=q.device, dtype=torch.int32), cu[1:], right=True).clamp(max=B - 1)
        km = cache.k_mean.index_select(0, seq)                                      # [total, Hkv, D]
        km = torch.repeat_interleave(km, Hq // cache.Hkv, dim=1)                    # [total, Hq, D]
        corr = torch.matmul(q.unsqueeze(2), km.unsqueeze(3)).reshape(total, Hq).to(torch.float32)
        lse = lse + corr.transpose(0, 1) * sm_scale
    return o, lse
