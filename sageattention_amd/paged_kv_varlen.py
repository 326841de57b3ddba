"""Packed, variable-length queries and appends on the paged quantised KV cache (gfx950 extension).

:func:`~sageattention_amd.kv_cache.sageattn_kvcache` and :meth:`PagedQuantizedKVCache.append` take dense operands with one length for all.  A
continuous-batching step holds one row for each decoding sequence, a few hundred rows for each prefill chunk and none for an idle slot, packed
as ``[total_tokens, H, D]`` behind ``cu_seqlens``.  The two functions here are those two calls on such operands -- the shape of
``flash_attn_varlen_func(..., block_table=, seqused_k=)`` -- so that an engine calls the library once per step, without padding, without a
call per distinct length and without a length on the host:

* :func:`append_varlen` appends each sequence's stretch of the packed new keys and values (``sage_kvpvarlen_append``);
* :func:`sageattn_kvcache_varlen` attends each sequence's stretch of the packed queries to that sequence's keys (``sage_kvpvarlen_attn``).

Per work item the kernels run what the dense calls run for that sequence's own row count: the outputs are bit for bit those of
``sageattn_kvcache(..., is_causal=True, causal_align="bottom_right")`` on the sequence's rows, and a cache filled by :func:`append_varlen` holds
byte for byte what ``append`` of the zero-padded rows with ``new_lens`` gives.  A malformed ``cu_seqlens`` gives wrong numbers, never an
access outside the packed tensors: every word is clamped on the device before it forms an address.

Import from here; the names are not part of the package's ``__all__``.  Not under torch.compile.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _cabi, _cabi_kvpvarlen, core, ops
from .kv_cache import _is_int
from .paged_kv_cache import PagedQuantizedKVCache
from .quant import _aligned, _dtype_code, _p, _stream

__all__ = ["sageattn_kvcache_varlen", "append_varlen"]


def _paged(name: str, cache) -> None:
    if not isinstance(cache, PagedQuantizedKVCache):
        raise ValueError(f"{name} takes a PagedQuantizedKVCache (got {type(cache).__name__}): the contiguous QuantizedKVCache has no packed route")
    if not cache._seeded:
        raise ValueError("the cache has no statistics yet: seed(k_mean, v_amax) or from_prefill(...) first")


def _prefix(name: str, cu, B: int, device) -> torch.Tensor:
    if not isinstance(cu, torch.Tensor) or cu.dtype != torch.int32:
        raise ValueError(f"{name} must be an int32 tensor (got {getattr(cu, 'dtype', type(cu).__name__)})")
    if cu.dim() != 1 or cu.shape[0] != B + 1:
        raise ValueError(f"{name} must have shape [B + 1] = [{B + 1}] (got {tuple(cu.shape)})")
    if cu.device != device:
        raise ValueError(f"{name} must be on the cache's device {device} (got {cu.device})")
    return cu.contiguous()


def _packed(name: str, t, H: Optional[int], cache) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 3:
        raise ValueError(f"{name} must be a 3-D tensor [total, H, D] (got {type(t).__name__} {list(getattr(t, 'shape', ()))})")
    if t.dtype != cache.dtype:
        raise ValueError(f"{name} must have the cache's dtype {cache.dtype} (got {t.dtype})")
    if t.device != cache.device:
        raise ValueError(f"{name} must be on the cache's device {cache.device} (got {t.device})")
    if t.shape[0] < 1 or t.shape[2] != cache.D or (H is not None and t.shape[1] != H):
        raise ValueError(f"{name} must be [total >= 1, {'Hq' if H is None else H}, {cache.D}] (got {list(t.shape)})")


def _host_max(name: str, x) -> int:
    if not _is_int(x) or x < 1:
        raise ValueError(f"{name} must be a positive int on the host (got {x!r})")
    return x


@torch.compiler.disable
def append_varlen(cache, k_new: torch.Tensor, v_new: torch.Tensor, cu_seqlens: torch.Tensor, max_new: int) -> None:
    """Append packed rows to a :class:`PagedQuantizedKVCache`: ``k_new`` / ``v_new`` ``[total, Hkv, D]`` in the cache's dtype, ``cu_seqlens``
    int32 ``[B + 1]`` on the device -- sequence b takes rows ``cu_seqlens[b] .. cu_seqlens[b + 1] - 1`` -- and ``max_new``, a host int that
    sizes the grid: a sequence takes at most ``max_new`` rows of its stretch.  Everything else is :meth:`PagedQuantizedKVCache.append`'s: rows
    that do not fit into the logical capacity are dropped on the device, a block whose page id lies outside the pool is not written, ``lens``
    advance.  Two launches on the current stream, no host read, no synchronisation: the call captures into a HIP graph and a replay follows
    the contents of ``cu_seqlens``, the rows and the table."""
    if torch.compiler.is_compiling():
        raise ValueError("append_varlen is not supported under torch.compile")
    _paged("append_varlen", cache)
    _packed("k_new", k_new, cache.Hkv, cache)
    _packed("v_new", v_new, cache.Hkv, cache)
    if k_new.shape != v_new.shape:
        raise ValueError(f"k_new and v_new must have one shape (got {list(k_new.shape)}, {list(v_new.shape)})")
    cu = _prefix("cu_seqlens", cu_seqlens, cache.B, cache.device)
    max_new = _host_max("max_new", max_new)
    k_new, v_new = _aligned(k_new, 8), _aligned(v_new, 8)
    rc = _cabi_kvpvarlen.load().sage_kvpvarlen_append(
        _p(cache.k_int8), _p(cache.k_scale), _p(cache.v_image), _p(cache.v_scale), _p(cache.v_amax), _p(cache.k_mean), _p(cache.k_tail),
        _p(cache.v_tail), _p(cache.lens), _p(k_new), _p(v_new), _p(cu), cache.B, cache.Hkv, int(k_new.shape[0]), max_new, cache.D,
        k_new.stride(0), k_new.stride(1), v_new.stride(0), v_new.stride(1), _dtype_code(k_new),
        _p(cache.block_table), cache.block_table.stride(0), cache.num_pages, cache.page_size, cache.max_pages_per_seq, _stream(k_new))
    _cabi.check(rc, "sage_kvpvarlen_append")


@torch.compiler.disable
def sageattn_kvcache_varlen(q: torch.Tensor, cache, cu_seqlens_q: torch.Tensor, max_seqlen_q: int, q_start=None, window_size=None,
                            pack_gqa=False, num_splits=None, sm_scale: Optional[float] = None, return_lse: bool = False):
    """Causal attention of packed queries to a :class:`PagedQuantizedKVCache`: ``q`` ``[total, Hq, D]`` in the cache's dtype, ``cu_seqlens_q``
    int32 ``[B + 1]`` on the device -- sequence b owns rows ``cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1`` and attends to its first
    ``cache.lens[b]`` keys -- and ``max_seqlen_q``, a host int that sizes the grid.

    The call is always causal.  With ``q_start=None`` it is aligned bottom-right: row i of sequence b stands at key ``cache.lens[b] - Lq_b +
    i``, FlashAttention's convention after the step's new tokens have been appended.  ``q_start`` (an int, or an int32 / int64 tensor ``[B]`` on
    the device) places row 0 of each sequence itself, as on :func:`~sageattention_amd.kv_cache.sageattn_kvcache`.  ``window_size=(left, 0)``
    means what it means there.  The offsets are formed by torch ops on the device; nothing is read on the host and nothing synchronises.

    Returns ``o`` ``[total, Hq, D]``; with ``return_lse`` also ``lse`` fp32 ``[Hq, total]`` in natural-log units, the layout and units of
    ``sageattn_qk_int8_pv_fp8_varlen``, with the K-mean correction of each token's own sequence when the cache smooths K.  Rows no sequence
    owns are not written.  **Rows of a sequence beyond ``max_seqlen_q`` are not computed** (neither ``o`` nor ``lse`` is written for them),
    and an idle slot (``Lq_b = 0``) costs ``Hq * ceil(max_seqlen_q / 128)`` workgroups that leave at once.  Each sequence's rows are bit for
    bit those of ``sageattn_kvcache(q_b, cache, is_causal=True, causal_align="bottom_right")`` (or with the same ``q_start`` / ``window_size``).

    Decode rows run one workgroup per query head here: ``pack_gqa`` and ``num_splits`` have no packed form and raise ValueError when set,
    as does a contiguous ``QuantizedKVCache``."""
    if torch.compiler.is_compiling():
        raise ValueError("sageattn_kvcache_varlen is not supported under torch.compile")
    _paged("sageattn_kvcache_varlen", cache)
    if not (pack_gqa is None or pack_gqa is False):
        raise ValueError(f"pack_gqa is not supported by sageattn_kvcache_varlen (got {pack_gqa!r}): packed query rows run one workgroup per query head")
    if not (num_splits is None or (_is_int(num_splits) and num_splits == 1)):
        raise ValueError(f"num_splits is not supported by sageattn_kvcache_varlen (got {num_splits!r}): the split serves dense calls of one query block")
    _packed("q", q, None, cache)
    total, Hq, D = q.shape
    if Hq % cache.Hkv != 0:
        raise ValueError(f"num_qo_heads ({Hq}) must be divisible by the cache's num_kv_heads ({cache.Hkv})")
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
    rc = _cabi_kvpvarlen.load().sage_kvpvarlen_attn(
        _p(q), _p(cache.k_int8), _p(cache.v_image), _p(o), _p(lse), _p(cache.k_scale), _p(cache.v_scale), _p(cache.lens), _p(cu),
        _p(cache.block_table), cache.block_table.stride(0), cache.num_pages, cache.page_size, cache.max_pages_per_seq,
        B, Hq, cache.Hkv, total, max_seqlen_q, D, q.stride(0), q.stride(1),
        cache.k_int8.stride(0), cache.k_int8.stride(1), cache.k_int8.stride(2), o.stride(0), o.stride(1), total,
        1, core._sm_log2(sm_scale), code, code, _stream(q), _cabi.attr_arg(attr))
    ops.attn_check(rc, "sage_kvpvarlen_attn", attr, q.device)
    if not return_lse:
        return o
    lse = lse / 1.44269504                 # kernel LSE: log2 units
    if cache.k_mean is not None:
        # q . km^T per (query head, packed row) with the mean of the row's own sequence, in the input dtype as core._lse_correction forms it
        # (a row's sequence: the number of sequence ends at or in front of it -- a search, no synchronisation, and in range whatever
        #  cu_seqlens_q holds, where repeat_interleave(output_size=total) needs a prefix array that sums to total; rows no sequence owns
        #  take some sequence's mean, and their lse is not written anyway)
        seq = torch.bucketize(torch.arange(total, device=q.device, dtype=torch.int32), cu[1:], right=True).clamp(max=B - 1)
        km = cache.k_mean.index_select(0, seq)                                      # [total, Hkv, D]
        if Hq != cache.Hkv:
            km = torch.repeat_interleave(km, Hq // cache.Hkv, dim=1)                # [total, Hq, D]
        corr = torch.matmul(q.unsqueeze(2), km.unsqueeze(3)).reshape(total, Hq).to(torch.float32)
        lse = lse + corr.transpose(0, 1) * sm_scale
    return o, lse
