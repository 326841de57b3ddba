"""The FP8-PV attention arithmetic with a VISIBILITY PREDICATE ``[Lq, Lk]`` in place of the causal flag -- TEST INFRASTRUCTURE ONLY.

``tests/ref_fp8_torch.py::attn_fp8`` restated for any mask shape that a row-by-key predicate describes (a sliding window, a shifted
diagonal, a key length), vectorised over the query heads of one sample.  The arithmetic is that function's, step for step: the row maximum
as ``fma(S, scale, -8.807)`` over the visible scores, ``P = exp2(fma(S, scale, -m))``, the FP32 row sum of the unrounded P, P to e4m3
saturating, the tile product from a zero accumulator folded into ``O = O * alpha + T``, 64-key tiles in ascending order.  Two changes:
``l`` starts at 0 (``attn_fp8`` starts it at 1 and relies on the first rescale being exactly 0 -- the same number for a row that sees a
key), and a row that never sees a key returns ``o = +0``, ``lse = -inf``.  A tile in which a row sees nothing leaves that row's state as
it is (m unchanged, alpha = 1, P = 0), so tiles no row of a query block sees are skipped.

The C oracle's own mask arguments are no substitute: its masked path takes the unfused score form, one fp16 ulp of ``o`` away from its
causal path on the same inputs.  ``tests/test_window_host.py`` pins this restatement to the oracle's causal path with predicates the oracle
can express.  Nothing here imports ``sageattention_amd``.
"""
from __future__ import annotations

import numpy as np
import torch

from ref_fp8_torch import CTA_K, CTA_Q, S_FP8_OFFSET, _e4m3_satfinite, _exp2_32, _fma32


# The windowed GPU cases (tests/test_gpu_window.py), all causal: (len, offset s, window W) -- two batches of six samples.  What each reaches:
# DESIGN.md 3.11.  Shapes: Lk = 640 padded keys, Lq = 200 query rows.
LK, LQ = 640, 200
WINDOW_CASES = ((640, 440, 400), (640, 384, 256), (577, 377, 64), (640, 440, 37), (640, 300, 1), (640, 0, 128),
                (130, -70, 50), (200, 250, 100), (130, 300, 100), (640, 700, 100), (640, 1000, 100), (0, 5, 64))


def rows_without_keys(Lq: int, s: int, W: int, length: int) -> int:
    """Closed form: row i sees a key iff length >= 1 and max(0, -s) <= i <= length + W - 2 - s (``W = 0``, unbounded: no upper limit)."""
    if length < 1:
        return Lq
    first, last = max(0, -s), (min(Lq - 1, length + W - 2 - s) if W > 0 else Lq - 1)
    return Lq - max(0, last - first + 1)


def visible(Lq: int, Lk: int, s: int, W: int, r: int, length: int) -> torch.Tensor:
    """The definition: row i attends to key j iff ``s + r + i - W < j <= s + r + i`` and ``0 <= j < clamp(length, 0, Lk)``.
    ``W = 0``: unbounded look-back."""
    i = torch.arange(Lq, dtype=torch.int64)[:, None]
    j = torch.arange(Lk, dtype=torch.int64)[None, :]
    keep = (j <= s + r + i) & (j < max(0, min(length, Lk)))
    if W > 0:
        keep &= j > s + r + i - W
    return keep


def visible_from_keywords(Lq: int, Lk: int, window_size, is_causal: bool, q_start: int, length: int) -> torch.Tensor:
    """The same predicate from the public keywords: ``window_size=(left, right)`` in FlashAttention's convention (-1 = unbounded on that
    side) relative to the diagonal ``j = q_start + i``."""
    left, right = window_size
    if is_causal:
        right = 0
    i = torch.arange(Lq, dtype=torch.int64)[:, None]
    j = torch.arange(Lk, dtype=torch.int64)[None, :]
    d = j - (q_start + i)                                    # key position relative to the row's diagonal
    keep = (j < max(0, min(length, Lk))).expand(Lq, Lk)      # ([Lq, Lk] also when both sides are unbounded and no row-dependent term follows)
    if right >= 0:
        keep = keep & (d <= right)
    if left >= 0:
        keep = keep & (d >= -left)
    return keep


def attn_window(q8, k8, v8, q_scale, q_slot, k_scale, k_slot, v_scale, keep, *, c, out_dtype: torch.dtype):
    """One sample, every query head at once.  q8 [Hq, Lq, D] int8, k8 [Hkv, Lk, D] int8, v8 [Hkv, Lk, D] e4m3 bytes (uint8); q_scale
    [Hq, nq] / k_scale [Hkv, nk] the slot vectors, q_slot [Lq] / k_slot [Lk] the slot of every row; v_scale [Hkv, D]; ``keep`` [Lq, Lk]
    bool; ``c`` = fl32(sm_scale) * fl32(log2 e).  numpy arrays or torch tensors.  Returns (o [Hq, Lq, D] ``out_dtype``, lse [Hq, Lq] fp32,
    log2 units)."""
    t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    q8, k8, v8, q_scale, k_scale, v_scale, keep = (t(a) for a in (q8, k8, v8, q_scale, k_scale, v_scale, keep))
    q_slot, k_slot = t(q_slot).long(), t(k_slot).long()
    Hq, Lq, D = q8.shape
    Hkv, Lk = k8.shape[0], k8.shape[1]
    g = Hq // Hkv
    k8 = k8.repeat_interleave(g, 0)
    vf = v8.view(torch.float8_e4m3fn).float().repeat_interleave(g, 0)             # [Hq, Lk, D]
    k_scale, v_scale = k_scale.repeat_interleave(g, 0), v_scale.repeat_interleave(g, 0)
    sm = torch.tensor(c, dtype=torch.float32)
    o = torch.zeros(Hq, Lq, D, dtype=out_dtype)
    lse = torch.full((Hq, Lq), -float("inf"), dtype=torch.float32)
    ninf = torch.tensor(-float("inf"))
    for r0 in range(0, Lq, CTA_Q):
        rows = min(CTA_Q, Lq - r0)
        qi = q8[:, r0:r0 + rows].double()
        qs = q_scale[:, q_slot[r0:r0 + rows]]                                       # [Hq, rows]
        m = torch.full((Hq, rows), -5000000.0)
        d = torch.zeros(Hq, rows)
        RO = torch.zeros(Hq, rows, D)
        for n0 in range(0, Lk, CTA_K):
            nk = min(CTA_K, Lk - n0)
            kp = keep[r0:r0 + rows, n0:n0 + nk]
            if not bool(kp.any()):
                continue
            kp = kp[None]
            S = (qi @ k8[:, n0:n0 + nk].double().transpose(1, 2)).float()           # exact integers
            scale = sm * (qs[:, :, None] * k_scale[:, k_slot[n0:n0 + nk]][:, None, :])
            m_temp = torch.where(kp, _fma32(S, scale, -S_FP8_OFFSET), ninf).amax(dim=2)
            m_new = torch.maximum(m, m_temp)
            o_scale = _exp2_32(m - m_new)
            P = torch.where(kp, _exp2_32(_fma32(S, scale, -m_new[:, :, None])), torch.tensor(0.0))
            rs = torch.zeros(Hq, rows)
            for j in range(nk):
                rs = rs + P[:, :, j]
            d = d * o_scale + rs
            P8 = _e4m3_satfinite(P).float()
            T = torch.zeros(Hq, rows, D)
            for j in range(nk):
                T = T + P8[:, :, j:j + 1] * vf[:, n0 + j][:, None, :]
            RO = RO * o_scale[:, :, None] + T
            m = m_new
        seen = d > 0
        x = (RO / torch.where(seen, d, torch.tensor(1.0))[:, :, None]) * v_scale[:, None, :]
        o[:, r0:r0 + rows] = torch.where(seen[:, :, None], x, torch.tensor(0.0)).to(out_dtype)
        lse[:, r0:r0 + rows] = torch.where(seen, torch.log2(d) + m, ninf)
    return o, lse
