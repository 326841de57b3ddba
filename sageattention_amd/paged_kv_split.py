"""Exact split-KV (``num_splits``) on the quantised KV caches, the paged one included (gfx950 extension).

:func:`~sageattention_amd.kv_cache.sageattn_kvcache` takes ``num_splits`` on a contiguous
:class:`~sageattention_amd.kv_cache.QuantizedKVCache` and refuses it on a
:class:`~sageattention_amd.paged_kv_cache.PagedQuantizedKVCache`.  :func:`sageattn_kvcache_split` takes it on both: on the paged cache the call
is ``sage_kvpsplit_attn`` (include/sage_kvpsplit_gfx950.h) -- the split's two passes looking their tiles up in the block table, then the merge --
and returns, bit for bit, what the contiguous cache of the same content and capacity returns with the same ``num_splits``.

Import from here (``from sageattention_amd.paged_kv_split import sageattn_kvcache_split``); the name is not part of the package's ``__all__``.
Not under torch.compile.
"""
from __future__ import annotations

from typing import Optional

import torch

from .kv_cache import _attend

__all__ = ["sageattn_kvcache_split"]


@torch.compiler.disable
def sageattn_kvcache_split(q: torch.Tensor, cache, num_splits, tensor_layout: str = "HND", is_causal: bool = False, causal_align: str = "top_left",
                           q_start=None, pack_gqa=False, sm_scale: Optional[float] = None, return_lse: bool = False):
    """:func:`~sageattention_amd.kv_cache.sageattn_kvcache` ``(q, cache, ..., num_splits=num_splits)`` on either kind of cache.

    ``num_splits`` means what it means for ``sageattn_qk_int8_pv_fp8_cuda``: an int in ``[2, 255]`` runs the call (one query block, ``Lq <=
    128``) as that many chunks of the key range, exactly; ``1`` / ``None`` is the unsplit call; ``"auto"`` / ``0`` plans the chunk count from
    the shapes, the cache's logical capacity standing for the key length.  The other keywords go through the family's one resolver and raise
    its ValueErrors in its order; ``window_size`` is not offered (a window bounds the keys itself).  On a paged cache a chunk is
    ``ceil(ceil(capacity / 64) / num_splits)`` tiles of the logical key axis and need not start on a page boundary; only the table entries of
    a chunk's own tiles in front of ``ceil(lens[b] / 64)`` are read.  No host read of lengths, offsets or the table, no synchronisation: the
    call captures into a HIP graph."""
    return _attend("sageattn_kvcache_split", q, cache, tensor_layout, is_causal, causal_align, q_start, None, pack_gqa, num_splits, sm_scale,
                   return_lse, True)
