"""Reference side of the packed route's bottom-right causal alignment (``sageattn_qk_int8_pv_fp8_varlen(causal_align="bottom_right")``).

Row i of sequence b (Lq_b rows, Lk_b keys, s_b = Lk_b - Lq_b) attends to key j of that sequence iff ``j <= i + s_b``.  Three things live here,
shared by tests/test_varlen_br_host.py (CPU) and tests/test_gpu_varlen_br.py (GPU):

  * ``visible`` / ``rows_without_keys``: the predicate, key by key, and the closed form of the rows that see nothing;
  * ``loop_bounds``: the attention kernel's loop bounds for one work item (sage_attn_kernel.h, CAUSAL and QSTART with kchunk0 = Lq - Lk, 64-key
    tiles), restated in Python with C's truncating division, and ``item_weight``, the work list's weight of that item;
  * ``oracle_f8_varlen_br``: the exact CPU oracle of the packed FP8 route with the shift restated by padding -- the oracle has no offset
    argument.  For s >= 0, s zero rows go in front of q8 with the group index given explicitly (the real rows keep their 128-row scale groups),
    the top-left causal oracle runs and the last Lq rows are kept; for s < 0 the first -s rows are +0 / -inf and the rest is the top-left
    oracle on the remaining rows with their original groups.  Either way the oracle walks the keys in 64-key tiles from key 0, as the kernel does.
"""
import numpy as np

BLKQ, BLKK = 128, 64


# ---------------------------------------------------------------------------------------------- the definition
def visible(lq: int, lk: int) -> np.ndarray:
    """bool [lq, lk]: row i sees key j."""
    i = np.arange(lq)[:, None]
    j = np.arange(lk)[None, :]
    return j <= i + (lk - lq)


def rows_without_keys(lq: int, lk: int) -> int:
    """The first max(0, Lq - Lk) rows of a sequence see nothing; with no keys at all, every row."""
    return lq if lk == 0 else min(lq, max(0, lq - lk))


# ---------------------------------------------------------------------------------------------- the kernel's loop bounds
def _cdiv(a: int, b: int) -> int:
    """C's integer division: truncation towards zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def loop_bounds(lq: int, lk: int, qblk: int) -> dict:
    """What sage_attn_kernel computes for query block ``qblk`` of a sequence under the bottom-right mask: ``n_iters`` 64-key tiles run in all;
    the first ``n_steady`` (when positive) run unmasked in the pipelined loop; ``diag_ok``: the two tiles behind them take the pipelined
    last-tile bodies, else every tile from max(n_steady, 0) on is a general (masked) iteration."""
    kchunk0 = -(lk - lq)
    n_iters = _cdiv(lk + BLKK - 1, BLKK)
    lim = max(_cdiv(qblk * BLKQ + BLKQ - kchunk0 + BLKK - 1, BLKK), 0)
    n_iters = min(lim, n_iters)
    n_steady = min(lk // BLKK - 2, n_iters - 2)
    nd = max(_cdiv(qblk * BLKQ - kchunk0, BLKK), 0)
    n_steady = min(n_steady, nd)
    diag_ok = (kchunk0 & (BLKK - 1)) == 0 and ((n_iters - n_steady == 2) if n_steady > 0 else (n_iters == 2 and lk >= 2 * BLKK))
    return dict(kchunk0=kchunk0, n_iters=n_iters, n_steady=n_steady, nd=nd, diag_ok=diag_ok)


def item_weight(lq: int, lk: int, j: int) -> int:
    """clamp(ceil((Lk - Lq + 128 (j + 1)) / 64), 0, ceil(Lk / 64)): the tiles the kernel's ``lim`` gives query block j."""
    return min(max(-((-(lk - lq + BLKQ * (j + 1))) // BLKK), 0), -(-lk // BLKK))


# ---------------------------------------------------------------------------------------------- the oracle, shifted by padding
def oracle_f8_varlen_br(O, q, k, v, dt, cu_q, cu_k, *, km, sm_scale=None, return_lse=False):
    """The packed FP8 route (per-block INT8 Q with sm_scale log2(e) folded in, per-block INT8 K smoothed by ``km``, e4m3 V with one scale per
    (sequence, kv head, channel), two-level accumulation, the exact score form) under the bottom-right mask, on bit arrays [sum L, H, D].
    ``km``: bits [1, Hkv, D] or None.  Returns (o bits [sum Lq, Hq, D0], lse [Hq, sum Lq] in natural-log units, or None).  Rows that see
    nothing are +0 / -inf exactly."""
    D0 = q.shape[-1]
    q, k, v = (O._pad_head_dim(t, dt) for t in (q, k, v))
    Hq, Hkv, D = q.shape[1], k.shape[1], q.shape[2]
    if sm_scale is None:
        sm_scale = 1.0 / (D0 ** 0.5)
    kind = "f16" if dt == 0 else "bf16"
    if km is not None:
        kmp = np.zeros((1, Hkv, D), dtype=np.uint16)
        kmp[..., :D0] = np.asarray(km).reshape(1, Hkv, -1)[..., :D0]
        k = O.convert(O.to_f32(k, dt) - O.to_f32(kmp, dt), kind)
    o = np.zeros(q.shape, dtype=np.uint16)
    lse = np.full((Hq, q.shape[0]), -np.inf, dtype=np.float32)
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        lq, lk = q1 - q0, k1 - k0
        s = lk - lq
        front, drop = max(0, s), max(0, -s)
        if lq == 0 or lk == 0 or drop >= lq:
            continue
        qb = np.ascontiguousarray(q[q0:q1].transpose(1, 0, 2))[None]
        kb = np.ascontiguousarray(k[k0:k1].transpose(1, 0, 2))[None]
        vb = np.ascontiguousarray(v[k0:k1].transpose(1, 0, 2))[None]
        gq, nq = O.group_index(lq, "per_block", "q", BLKQ, BLKQ)
        gk, nk = O.group_index(lk, "per_block", "k", BLKK, BLKK)
        q8, qsc = O.quant_int8(qb, dt, gq, nq, pre_scale=np.float32(sm_scale * O.LOG2E), style=O.STYLE_TRITON)
        k8, ksc = O.quant_int8(kb, dt, gk, nk, style=O.STYLE_TRITON)
        v8, vs = O.quant_v_fp8(vb, dt)
        q8s = np.ascontiguousarray(np.concatenate([np.zeros((1, Hq, front, D), np.int8), q8[:, :, drop:]], axis=2))
        gqs = np.concatenate([np.zeros(front, np.int32), gq[drop:]])
        ob, lb = O.attn(q8s, k8, v8, qsc, gqs, ksc, gk, causal=True, c=1.0, pv_mode=O.PV_F8_TWO_LEVEL, out_dtype=dt, v_scale=vs,
                        return_lse=True, score_mode=O.SCORES_EXACT)
        o[q0 + drop:q1] = ob[0, :, front:].transpose(1, 0, 2)
        lse[:, q0 + drop:q1] = lb[0, :, front:]
    if not return_lse:
        return np.ascontiguousarray(o[..., :D0]), None
    lse = lse / np.float32(O.LOG2E)
    if km is not None:            # q . km per (head, row) in the input dtype, * sm_scale, as the call's own correction
        kmq = np.repeat(O.to_f32(np.asarray(km).reshape(1, Hkv, -1), dt)[0, :, :D0], Hq // Hkv, axis=0)
        corr = np.einsum("thd,hd->ht", O.to_f32(q[..., :D0], dt), kmq)
        lse = lse + O.to_f32(O.convert(corr.astype(np.float32), kind), dt) * np.float32(sm_scale)
    return np.ascontiguousarray(o[..., :D0]), lse
