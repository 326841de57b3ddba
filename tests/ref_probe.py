"""V as a measuring instrument: probe values that make an attention output spell out WHICH KEYS each row attended to -- TEST
INFRASTRUCTURE ONLY.

Channel ``d`` of the probe V has one non-zero row, the row of key ``j0 + d``, holding 1.0.  Then ``o[i, d]`` is the attention weight of row
``i`` on key ``j0 + d`` -- exactly ``+0`` iff the key is invisible, whatever the arithmetic of the route (a sum of zeros is zero; a visible
key's P is a normal number under the conditions below, so its weight is positive).  A sweep ``j0 = 0, D, 2D, ...`` reads the ``Lq x Lk``
visibility matrix as booleans, with no tolerance, and the weights themselves to the precision of the route's P format.

Signature holes: the channels with ``d % 16 == sig[h]`` stay all zero, ``sig`` distinct for every (sample, kv-head) of a call (so
``B * Hkv <= 16``).  A hole must read ``+0`` in every row, every other channel follows the predicate: a route that reads V of another
sample, another kv-head or another sequence of a packed batch shows a weight in a hole, or a hole where a weight belongs.  The keys of the
hole channels are not read by that sweep; a second sweep with the signatures moved by 8 reads them (``sweeps``).

  * ``probe_v`` / ``probe_v_packed``: the operand;
  * ``read_visibility``: the decoder -- what was seen, which keys the sweep could read, the weights, and the list of violations;
  * ``weights_fp64`` / ``score_spread``: the FP64 softmax over the visible keys of the scores ``q8 . k8 * q_scale * k_scale * c`` of the
    oracle's quantised operands (``aux`` of ``oracle.sageattn_dense``), and the largest per-row spread of the visible scores in log2 units;
  * ``judge``: the assertions every test applies to one decoded sweep, in a fixed order, and the derived bars.

Nothing here imports ``sageattention_amd``.
"""
from __future__ import annotations

import numpy as np
import torch

# The derived bars: |got - w_ref| <= bar * w_ref + one output ulp at w_ref.  P rounded to nearest in its format (e4m3: 3 mantissa bits,
# half an ulp is 2^-4 relative; fp16: 2^-11), the output rounding (2^-8 covers bf16's half ulp with room), slack for the fp32 exp2 and
# sums (2^-10).  The row sum is of the unrounded P (FP8-PV) or unbiased (FP16-PV): no further term.
BAR_F8 = 2.0 ** -4 + 2.0 ** -8 + 2.0 ** -10
BAR_F16 = 2.0 ** -11 + 2.0 ** -8 + 2.0 ** -10
# The conditions under which a visible key cannot read as zero: every visible P is a normal e4m3 number (448 * 2^-6 = 7 >= 2^-6) and every
# visible weight a normal fp16 / bf16 number well above one ulp of the smallest.
MAX_SPREAD = 6.0
MIN_WEIGHT = 2.0 ** -12


def sweeps(D: int, n: int, B: int, Hkv: int):
    """The probe calls that read every key of ``n`` once or twice: ``(j0, sig)`` with ``sig[b][h]`` -- the sweep ``j0 = 0, D, ...`` with the
    signatures ``b * Hkv + h`` and the same sweep with the signatures moved by 8 (the first sweep's hole keys)."""
    assert B * Hkv <= 16, "one signature per (sample, kv-head) of a call: B * Hkv <= 16"
    out = []
    for shift in (0, 8):
        sig = [[(b * Hkv + h + shift) % 16 for h in range(Hkv)] for b in range(B)]
        out += [(j0, sig) for j0 in range(0, max(n, 1), D)]
    return out


def probe_v(Hkv: int, n: int, D: int, j0: int, sig, dtype: torch.dtype) -> torch.Tensor:
    """``[Hkv, n, D]``: ``v[h, j0 + d, d] = 1.0`` for ``j0 + d < n`` and ``d % 16 != sig[h]``, zero elsewhere."""
    assert len(sig) == Hkv and all(0 <= s < 16 for s in sig)
    v = torch.zeros(Hkv, n, D, dtype=dtype)
    for h in range(Hkv):
        for d in range(D):
            if d % 16 != sig[h] and 0 <= j0 + d < n:
                v[h, j0 + d, d] = 1.0
    return v


def probe_v_packed(Hkv: int, cu_seqlens_k, D: int, j0: int, sig, dtype: torch.dtype) -> torch.Tensor:
    """The packed variant ``[sum Lk, Hkv, D]``: sequence b's rows hold ``probe_v(Hkv, Lk_b, D, j0, sig[b])``, key positions counted from the
    sequence's own first key."""
    cu = [int(x) for x in cu_seqlens_k]
    v = torch.zeros(cu[-1], Hkv, D, dtype=dtype)
    for b in range(len(cu) - 1):
        v[cu[b]:cu[b + 1]] = probe_v(Hkv, cu[b + 1] - cu[b], D, j0, sig[b], dtype).transpose(0, 1)
    return v


def read_visibility(outputs_by_j0, n: int, sig, Hkv: int):
    """Decode one sample's sweep.  ``outputs_by_j0``: ``[(j0, o)]`` with ``o`` a float array ``[Hq, Lq, D]`` (the route's output for the
    probe of that ``j0``, all with the signatures ``sig`` ``[Hkv]``).  Returns ``(seen, known, weights, violations)``: ``seen`` bool
    ``[Hq, Lq, n]``, an entry is ``o > 0``; ``known`` bool ``[Hq, n]``, the keys some call of the sweep had a channel for; ``weights``
    float64 ``[Hq, Lq, n]``, the values read (0 where unknown); ``violations``: strings -- a negative, ``-0`` or non-finite value, a hole
    channel that is non-zero, a channel past ``n`` that is non-zero, a key read twice with two answers."""
    o0 = np.asarray(outputs_by_j0[0][1])
    Hq, Lq, D = o0.shape
    g = Hq // Hkv
    seen = np.zeros((Hq, Lq, n), dtype=bool)
    known = np.zeros((Hq, n), dtype=bool)
    weights = np.zeros((Hq, Lq, n), dtype=np.float64)
    bad = []
    for j0, o in outputs_by_j0:
        o = np.asarray(o)
        assert o.shape == (Hq, Lq, D)
        if not np.isfinite(o).all():
            bad.append(f"j0 {j0}: {int((~np.isfinite(o)).sum())} non-finite values")
        if np.signbit(o).any():
            bad.append(f"j0 {j0}: {int(np.signbit(o).sum())} values negative or -0")
        for h in range(Hq):
            for d in range(D):
                j, col = j0 + d, o[h, :, d]
                if d % 16 == sig[h // g]:
                    if col.any():
                        bad.append(f"j0 {j0} head {h}: hole channel {d} is non-zero in {int((col != 0).sum())} rows")
                elif j >= n:
                    if col.any():
                        bad.append(f"j0 {j0} head {h}: channel {d} (key {j} >= {n}) is non-zero in {int((col != 0).sum())} rows")
                else:
                    s = col > 0
                    if known[h, j] and not np.array_equal(seen[h, :, j], s):
                        bad.append(f"j0 {j0} head {h}: key {j} read twice with two answers")
                    seen[h, :, j], known[h, j], weights[h, :, j] = s, True, col.astype(np.float64)
    return seen, known, weights, bad


def scores_fp64(aux, b: int = 0) -> np.ndarray:
    """float64 ``[Hq, Lq, Lk]``: ``q8 . k8 * q_scale * k_scale * c`` of sample ``b`` of the oracle's ``aux`` (log2 units)."""
    q8, k8 = np.asarray(aux["q8"][b], dtype=np.float64), np.asarray(aux["k8"][b], dtype=np.float64)
    g = q8.shape[0] // k8.shape[0]
    qs = np.asarray(aux["qs"][b], dtype=np.float64)[:, np.asarray(aux["gq"])]                     # [Hq, Lq]
    ks = np.repeat(np.asarray(aux["ks"][b], dtype=np.float64)[:, np.asarray(aux["gk"])], g, axis=0)   # [Hq, Lk]
    s = np.einsum("hid,hjd->hij", q8, np.repeat(k8, g, axis=0))
    return s * qs[:, :, None] * ks[:, None, :] * float(aux["c"])


def weights_fp64(aux, keep, b: int = 0) -> np.ndarray:
    """float64 ``[Hq, Lq, Lk]``: the softmax (base 2: the scores are in log2 units) over the keys ``keep`` ``[Lq, Lk]`` marks visible; 0 at
    invisible keys and in rows that see nothing."""
    keep = np.asarray(keep, dtype=bool)
    s = np.where(keep[None], scores_fp64(aux, b), -np.inf)
    m = s.max(axis=2, keepdims=True)
    p = np.where(keep[None], np.exp2(s - np.where(np.isfinite(m), m, 0.0)), 0.0)
    l = p.sum(axis=2, keepdims=True)
    return p / np.where(l > 0, l, 1.0)


def score_spread(aux, keep, b: int = 0) -> float:
    """The largest per-row ``max - min`` of the visible scores, in log2 units (0 if no row sees a key)."""
    keep = np.asarray(keep, dtype=bool)
    s = scores_fp64(aux, b)
    hi = np.where(keep[None], s, -np.inf).max(axis=2)
    lo = np.where(keep[None], s, np.inf).min(axis=2)
    rows = keep.any(axis=1)
    return float((hi - lo)[:, rows].max()) if rows.any() else 0.0


def out_ulp(w: np.ndarray, code: int) -> np.ndarray:
    """One ulp of the output dtype (0: fp16, 1: bf16) at each ``w > 0`` (fp16 subnormals: 2^-24 apart); 0 at ``w == 0``."""
    w = np.asarray(w, dtype=np.float64)
    e = np.floor(np.log2(np.where(w > 0, w, 1.0)))
    ulp = np.exp2(e - (7 if code == 1 else 10))
    if code == 0:
        ulp = np.maximum(ulp, 2.0 ** -24)
    return np.where(w > 0, ulp, 0.0)


def check_conditions(w_ref: np.ndarray, keep, spread: float) -> None:
    """The conditions of the method, asserted on the reference alone: no visible key may be able to read as zero."""
    keep = np.asarray(keep, dtype=bool)
    assert spread <= MAX_SPREAD, f"score spread {spread:.2f} log2 units exceeds {MAX_SPREAD}: a visible P could leave e4m3's normal range"
    if keep.any():
        lo = float(w_ref[:, keep].min())
        assert lo >= MIN_WEIGHT, f"smallest visible reference weight {lo:.3e} is below 2^-12"


def judge(seen, known, weights, violations, keep, w_ref, bar: float, code: int, lse=None, what: str = "") -> float:
    """The assertions on one decoded sweep, in order: (1) the visibility read back is the predicate, exactly, on every key the sweep read;
    no violation; rows that see nothing have ``lse = -inf``, all others a finite one (``lse`` ``[Hq, Lq]`` or None); (2) each non-empty
    row's weights -- the unread keys' taken from the reference -- sum to 1 within ``bar`` plus one output ulp per visible key; (3) every
    visible weight read is within ``bar * w_ref`` plus one output ulp at ``w_ref``.  Returns the largest ``err / (bar * w_ref)``."""
    keep = np.asarray(keep, dtype=bool)
    Hq, Lq, n = seen.shape
    assert keep.shape == (Lq, n), (what, keep.shape, seen.shape)
    kn = np.broadcast_to(known[:, None, :], seen.shape)
    want = np.broadcast_to(keep[None], seen.shape)
    wrong = (seen != want) & kn
    if wrong.any():
        h, i, j = (int(x[0]) for x in np.nonzero(wrong))
        raise AssertionError(f"{what}: {int(wrong.sum())} wrong entries of the visibility set, first: head {h} row {i} key {j} "
                             f"{'seen' if seen[h, i, j] else 'not seen'}, predicate says {'visible' if keep[i, j] else 'invisible'}")
    assert not violations, f"{what}: {len(violations)} violations, first: {violations[0]}"
    if lse is not None:
        lse = np.asarray(lse)
        empty = np.broadcast_to(~keep.any(axis=1), (Hq, Lq))
        assert not np.isnan(lse).any(), f"{what}: NaN in lse"
        assert np.array_equal(np.isneginf(lse), empty) and np.isfinite(lse[~empty]).all(), f"{what}: lse = -inf in other rows than the predicate's empty ones"
    ulp = out_ulp(w_ref, code)
    total = np.where(kn, weights, w_ref).sum(axis=2)
    rows = np.broadcast_to(keep.any(axis=1), (Hq, Lq))
    off = np.abs(total - 1.0)[rows]
    room = (bar + np.where(want, ulp, 0.0).sum(axis=2))[rows]
    assert (off <= room).all(), f"{what}: a row's weights sum to 1 +- {float(off.max()):.3e}"
    sel = want & kn
    err = np.abs(weights - w_ref)[sel]
    ratio = float((err / (bar * w_ref[sel])).max()) if sel.any() else 0.0
    over = err > bar * w_ref[sel] + ulp[sel]
    assert not over.any(), (f"{what}: {int(over.sum())} visible weights outside bar {bar:.4f} * w_ref + 1 ulp; "
                            f"largest err / (bar * w_ref) = {ratio:.3f}")
    return ratio


# ---------------------------------------------------------------------------------------------- what the host and the GPU file share
# (D, dtype, layout); 96 only where the route takes it.
CASES = ((64, torch.float16, "HND"), (128, torch.bfloat16, "NHD"), (96, torch.float16, "HND"))
CASE_IDS = ("d64-f16-HND", "d128-bf16-NHD", "d96-f16-HND")
HQ, HKV, LQ, LK = 4, 2, 200, 320
# (len, q_start, W): windows that start and end on, one before and one after a 64-key boundary, a diagonal left of key 0, rows past the
# last key, a single key, no key.  W = 0: unbounded look-back.
TRIPLES = ((320, 120, 0), (320, 120, 65), (257, 57, 64), (193, 130, 37), (130, -70, 50), (64, 300, 1), (1, 0, 0), (0, 5, 64))
BATCH_OFFSETS = (0, 2, 3, 4, 6, 7)        # the six samples of a call without a window: (len, q_start) of these triples
BATCH_WINDOWS = (1, 2, 3, 4, 5, 7)        # the six samples of a windowed call
WINDOWS = (65, 64, 37, 50, 1)             # the windows of the triples, one per call: every sample of the batch is checked under each


def qk(B: int, Hq: int, Hkv: int, Lq: int, Lk: int, D: int, dtype: torch.dtype, seed: int):
    """``q = 0.5 randn`` ``[B, Hq, Lq, D]`` and ``k = randn + a per-channel offset`` ``[B, Hkv, Lk, D]`` (HND, on the host), fixed seed."""
    g = torch.Generator().manual_seed(seed)
    q = (0.5 * torch.randn(B, Hq, Lq, D, generator=g)).to(dtype)
    k = (torch.randn(B, Hkv, Lk, D, generator=g) + torch.randn(1, Hkv, 1, D, generator=g)).to(dtype)
    return q, k


def visible(Lq: int, n: int, s: int, W: int, r: int = 0, causal: bool = True) -> np.ndarray:
    """bool ``[Lq, n]``: row i sees key j iff ``s + r + i - W < j <= s + r + i`` (``W = 0``: no lower limit; not ``causal``: every key)."""
    i = np.arange(Lq, dtype=np.int64)[:, None]
    j = np.arange(n, dtype=np.int64)[None, :]
    if not causal:
        return np.ones((Lq, n), dtype=bool)
    keep = j <= s + r + i
    if W > 0:
        keep &= j > s + r + i - W
    return keep


# One seed per sample.  With 320 visible keys the conditions are tight (a row's visible scores spread over about six sigma of q . k), so
# each sample's seed is the first at which sample-sized ``qk`` meets them with room -- spread <= 5.75, smallest weight >= 2^-11.75 -- when
# every row sees all 320 keys, judged on the oracle's operands alone; every mask of the tests shows a row a subset of those keys, which
# narrows the spread and raises the weights.  The tests assert the conditions themselves for every mask they use.
SEEDS = {(64, "f16", 4, 200): (49, 648, 979, 1938, 2627, 3277), (64, "f16", 4, 16): (1, 2, 3, 4, 5, 6), (64, "f16", 8, 1): (0, 1, 2, 3, 4, 5),
         (64, "f16", 8, 17): (5, 9, 11, 19, 21, 24), (128, "bf16", 4, 200): (3, 7, 10, 22, 36, 43), (128, "bf16", 4, 16): (0, 3, 4, 5, 6, 7),
         (128, "bf16", 8, 1): (0, 1, 2, 3, 4, 5), (128, "bf16", 8, 17): (0, 1, 3, 5, 6, 7), (96, "f16", 4, 200): (220, 277, 296, 335, 407, 511)}


def operands(D: int, dtype: torch.dtype, Hq: int = HQ, Lq: int = LQ, B: int = 6):
    """``q`` ``[B, Hq, Lq, D]`` and ``k`` ``[B, HKV, LK, D]`` (HND, host), sample b drawn with its own seed of ``SEEDS``."""
    seeds = SEEDS[(D, "f16" if dtype == torch.float16 else "bf16", Hq, Lq)][:B]
    parts = [qk(1, Hq, HKV, Lq, LK, D, dtype, s) for s in seeds]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def dense_masks(Lq: int = LQ):
    """The masks of the dense FP8-PV calls, by name: six samples of ``(len, s, W, r, causal)`` each -- row i of the sample sees key j iff
    ``j < len`` and (``causal``) ``s + r + i - W < j <= s + r + i``.  What each name is as keywords: tests/test_gpu_visibility.py."""
    off = [TRIPLES[t][:2] for t in BATCH_OFFSETS]
    win = [TRIPLES[t][:2] for t in BATCH_WINDOWS]
    m = {"kv_lens": [(n, 0, 0, 0, False) for n, _ in off],
         "kv_lens-causal": [(n, 0, 0, 0, True) for n, _ in off],
         "q_start": [(n, s, 0, 0, True) for n, s in off],
         "bottom_right": [(n, n - Lq, 0, 0, True) for n, _ in off],
         "window(100,30)": [(n, s, 131, 30, True) for n, s in off],
         "window(-1,30)": [(n, s, 0, 30, True) for n, s in off]}
    for W in WINDOWS:
        m[f"window{W}"] = [(n, s, W, 0, True) for n, s in win]
    return m
