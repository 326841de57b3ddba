"""Reference side of the packed route's sliding window (``sageattn_qk_int8_pv_fp8_varlen(causal_align="bottom_right", window_size=...)``).

With ``Lq_b``, ``Lk_b`` from the prefix arrays, ``s_b = Lk_b - Lq_b`` and a window of ``W >= 1`` keys, row i of sequence b attends to key j
of that sequence iff ``s_b + i - W < j <= s_b + i`` and ``0 <= j < Lk_b`` (FlashAttention's varlen convention with ``W = left + 1``).
Shared by tests/test_varlen_window_host.py (CPU) and tests/test_gpu_varlen_window.py (GPU):

  * ``visible`` / ``visible_from_keywords`` / ``rows_without_keys``: the predicate from the kernel's parameters, from the public keywords, and
    the closed form of the rows that see nothing (W = 0: no window);
  * ``loop_bounds``: what sage_attn_kernel computes for one work item of the packed window form (WINDOW, QSTART, no KVLEN), restated next to
    ``ref_varlen_br.loop_bounds`` with C's truncating division -- the item's first key ``kc0``, the shifted length, ``lim``, the head tiles
    ``nh``, ``nd``, ``n_steady``, ``diag_ok`` -- and ``tiles_run``, which tile runs in which form;
  * ``ref_f8_varlen_window``: the packed FP8 route per sequence with a visibility predicate.  The operands are the oracle's (per-block INT8 Q
    with sm_scale log2(e) folded in and K smoothed by ``km``, both with Triton rounding; e4m3 V with one scale per (sequence, kv head,
    channel)); the attention arithmetic is ``ref_window.attn_window``'s: the exact score form, e4m3 P, two-level accumulation, ``l`` from 0, 64-key
    tiles from key 0 of the sequence -- the kernel's tiles too, since ``kc0`` is a multiple of 64 -- and rows without keys ``+0`` / ``-inf``.
    The C oracle has no window; tests/test_varlen_window_host.py pins this restatement to the oracle's packed causal path on the predicates
    that path can express.
"""
import numpy as np
import torch

import ref_window as rw
from ref_varlen_br import BLKK, BLKQ, _cdiv

W_MAX = 1 << 30


# ---------------------------------------------------------------------------------------------- the definition
def visible(lq: int, lk: int, W: int) -> np.ndarray:
    """bool [lq, lk]: row i sees key j.  W = 0: no window (the bottom-right causal mask)."""
    i = np.arange(lq, dtype=np.int64)[:, None]
    j = np.arange(lk, dtype=np.int64)[None, :]
    keep = j <= i + (lk - lq)
    if W > 0:
        keep &= j > i + (lk - lq) - W
    return keep


def visible_from_keywords(lq: int, lk: int, window_size) -> np.ndarray:
    """FlashAttention's varlen form of the same mask: key j is masked for row i iff ``j > i + Lk - Lq + right`` or ``j < i + Lk - Lq - left``
    (a negative side: unbounded), here with is_causal=True, i.e. right = 0."""
    left, right = window_size
    right = 0
    keep = np.ones((lq, lk), dtype=bool)
    for i in range(lq):
        for j in range(lk):
            if j > i + lk - lq + right or (left >= 0 and j < i + lk - lq - left):
                keep[i, j] = False
    return keep


def rows_without_keys(lq: int, lk: int, W: int = 0) -> int:
    """Row i sees a key iff Lk >= 1 and s + i >= 0: its window's last key is its diagonal, and the first key of a row on or behind key 0 lies
    in front of Lk.  The window never empties a row of its own: the first max(0, Lq - Lk) rows, or all without keys."""
    return lq if lk == 0 else min(lq, max(0, lq - lk))


# ---------------------------------------------------------------------------------------------- the kernel's loop bounds
def loop_bounds(lq: int, lk: int, W: int, qblk: int) -> dict:
    """sage_attn_kernel, packed window form, query block ``qblk`` of a sequence (Lq, Lk), window ``W`` (clamped to [1, 2^30] as the kernel
    clamps p.window).  Tile indices are relative to ``kc0``."""
    s = lk - lq
    wwin = 1 if W < 1 else min(W, W_MAX)
    a0 = (s - wwin) + qblk * BLKQ + 1
    kc0 = (a0 & ~(BLKK - 1)) if a0 > 0 else 0
    lk2 = lk - kc0 if lk > kc0 else 0
    kchunk0 = kc0 - s
    n_iters = _cdiv(lk2 + BLKK - 1, BLKK)
    lim = max(_cdiv(qblk * BLKQ + BLKQ - kchunk0 + BLKK - 1, BLKK), 0)
    n_iters = min(lim, n_iters)
    rlast = min(qblk * BLKQ + BLKQ - 1, lq - 1)
    x = rlast - kchunk0 + 1 - wwin
    nh = min((x + BLKK - 1) >> 6 if x > 0 else 0, n_iters)
    n_steady = min(_cdiv(lk2, BLKK) - 2, n_iters - 2)
    nd = max(_cdiv(qblk * BLKQ - kchunk0, BLKK), 0)
    n_steady = min(n_steady, nd)
    diag_ok = (kchunk0 & (BLKK - 1)) == 0 and ((n_iters - n_steady == 2) if n_steady > 0 else (n_iters == 2 and lk2 >= 2 * BLKK))
    diag_ok = diag_ok and nh <= max(n_steady, 0)
    return dict(kc0=kc0, lk=lk2, kchunk0=kchunk0, lim=lim, n_iters=n_iters, nh=nh, nd=nd, n_steady=n_steady, diag_ok=diag_ok, wwin=wwin)


def tiles_run(b: dict) -> dict:
    """Which tile (relative to kc0) runs in which form: ``head`` general iterations with the window comparison, ``steady`` unmasked in the
    pipelined loop, ``diag`` the pipelined last-tile bodies (causal mask only), ``general`` the remainder loop."""
    nh, ns, n = b["nh"], b["n_steady"], b["n_iters"]
    head = list(range(nh))
    steady = list(range(nh, ns)) if (nh < ns or b["diag_ok"]) else []
    at = max(nh, ns) if steady or b["diag_ok"] else nh
    diag = [at, at + 1] if b["diag_ok"] else []
    general = list(range(at + len(diag), n))
    return dict(head=head, steady=steady, diag=diag, general=general)


def sequence_kc0(lq: int, lk: int, W: int) -> int:
    """The first key any block of the sequence requests: block 0's ``kc0`` (ascending in the block index).  Keys, k scales and V images in
    front of it are never read."""
    return loop_bounds(lq, lk, W, 0)["kc0"] if lq > 0 else 0


# ---------------------------------------------------------------------------------------------- the arithmetic with a predicate
def ref_f8_varlen_window(O, q, k, v, dt, cu_q, cu_k, W, *, km, sm_scale=None, return_lse=False, keep_of=None):
    """Bit arrays [sum L, H, D] as ``ref_varlen_br.oracle_f8_varlen_br`` takes them.  ``keep_of(lq, lk)`` overrides the predicate (default:
    ``visible(lq, lk, W)``).  Returns (o bits [sum Lq, Hq, D0], lse [Hq, sum Lq] in natural-log units or None)."""
    D0 = q.shape[-1]
    q, k, v = (O._pad_head_dim(t, dt) for t in (q, k, v))
    Hq, Hkv, D = q.shape[1], k.shape[1], q.shape[2]
    if sm_scale is None:
        sm_scale = 1.0 / (D0 ** 0.5)
    kind = "f16" if dt == 0 else "bf16"
    tdt = torch.float16 if dt == 0 else torch.bfloat16
    if km is not None:
        kmp = np.zeros((1, Hkv, D), dtype=np.uint16)
        kmp[..., :D0] = np.asarray(km).reshape(1, Hkv, -1)[..., :D0]
        k = O.convert(O.to_f32(k, dt) - O.to_f32(kmp, dt), kind)
    o = np.zeros(q.shape, dtype=np.uint16)
    lse = np.full((Hq, q.shape[0]), -np.inf, dtype=np.float32)
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        lq, lk = q1 - q0, k1 - k0
        if lq == 0 or lk == 0:
            continue
        qb = np.ascontiguousarray(q[q0:q1].transpose(1, 0, 2))[None]
        kb = np.ascontiguousarray(k[k0:k1].transpose(1, 0, 2))[None]
        vb = np.ascontiguousarray(v[k0:k1].transpose(1, 0, 2))[None]
        gq, nq = O.group_index(lq, "per_block", "q", BLKQ, BLKQ)
        gk, nk = O.group_index(lk, "per_block", "k", BLKK, BLKK)
        q8, qsc = O.quant_int8(qb, dt, gq, nq, pre_scale=np.float32(sm_scale * O.LOG2E), style=O.STYLE_TRITON)
        k8, ksc = O.quant_int8(kb, dt, gk, nk, style=O.STYLE_TRITON)
        v8, vs = O.quant_v_fp8(vb, dt)
        keep = keep_of(lq, lk) if keep_of is not None else visible(lq, lk, W)
        ob, lb = rw.attn_window(q8[0], k8[0], v8[0], qsc[0], gq, ksc[0], gk, vs[0], keep, c=np.float32(1.0), out_dtype=tdt)
        o[q0:q1] = ob.view(torch.int16).numpy().view(np.uint16).transpose(1, 0, 2)
        lse[:, q0:q1] = lb.numpy()
    if not return_lse:
        return np.ascontiguousarray(o[..., :D0]), None
    lse = lse / np.float32(O.LOG2E)
    if km is not None:            # q . km per (head, row) in the input dtype, * sm_scale, as the call's own correction
        kmq = np.repeat(O.to_f32(np.asarray(km).reshape(1, Hkv, -1), dt)[0, :, :D0], Hq // Hkv, axis=0)
        corr = np.einsum("thd,hd->ht", O.to_f32(q[..., :D0], dt), kmq)
        lse = lse + O.to_f32(O.convert(corr.astype(np.float32), kind), dt) * np.float32(sm_scale)
    return np.ascontiguousarray(o[..., :D0]), lse
