"""The probe-V instrument (tests/ref_probe.py) for the wide FP8-PV entries -- ``hd256.sageattn_hd256``, ``qk192.sageattn_qk192``,
``qk192_varlen.sageattn_qk192_varlen``, ``mla_decode.sageattn_mla_decode`` -- TEST INFRASTRUCTURE ONLY.

What tests/test_gpu_visibility_wide.py (the kernels) and tests/test_probe_wide_host.py (the restatement and the negative controls) share:

  * the reference weights: the quantised operands of tests/ref_fp8_torch.py at the entry's padded width (``quant_int8_per_thread`` with
    ``groups(...)``, K against its own per-channel mean), packed as the ``aux`` mapping ``ref_probe.scores_fp64`` takes -- ``q8, k8, qs,
    ks, gq, gk`` and ``c = sm_scale * LOG2E`` (``dense_aux``, ``mla_aux``);
  * the restatement's own output on a probe (``restate``, ``restate_mla``: ``ref_fp8_torch.attn_fp8`` per head, the diagonal moved as
    tests/test_gpu_qk192_varlen.py moves it);
  * the engine (``run_probe``): conditions on the reference alone, then the sweeps, then ``ref_probe.judge`` in its fixed order;
  * the operand, case and seed tables.

The MLA entry has no free V: V is ``kv[..., :512]``.  It is made one by ``q[..., :512] = 0``: every INT8 product on the first 512
channels is then exactly 0, with or without ``smooth_k``, the score depends on the 64 rope channels only, and ``o[..., d]`` is the weight
on key ``j0 + d``.  The probe still moves the K scales (a row's abs-max is over all 576 channels), so the reference quantises the very
``kv`` a call gets: ``mla_aux`` is a function of the signatures.

``python tests/ref_probe_wide.py`` searches the seed table again and prints it.

Nothing here imports ``sageattention_amd``.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import ref_fp8_torch as ref
import ref_probe as rp

F16, BF16 = torch.float16, torch.bfloat16
B, HQ, HKV = 2, 4, 2
# (Lq, Lk): the top-left diagonal's end and the last key fall one after, on and one before a 64-key boundary
DENSE_SHAPES = ((200, 193), (129, 128), (65, 257))
# hd256: (D, dtype, layout); the probe has D channels, one ``j0`` call reads up to 240 keys at 256
HD256_CASES = ((256, F16, "HND"), (256, BF16, "NHD"), (192, BF16, "HND"), (192, F16, "NHD"))
# qk192 and its packed form: (Dqk, Dv, dtype, layout)
QK192_CASES = ((192, 128, F16, "HND"), (192, 128, BF16, "NHD"), (160, 64, BF16, "HND"), (160, 64, F16, "NHD"))
VARLEN_CASES = ((192, 128, F16), (160, 64, BF16))
# (Lq_s, Lk_s): a bottom-right shift of 63 and of -128, a sequence without rows, one tile exactly, one without keys at the end
SEQS = ((130, 193), (0, 70), (64, 64), (72, 200), (200, 72), (40, 0))
VARLEN_MASKS = ("none", "top_left", "bottom_right")
# MLA decode: B 3, Hkv 1 (the shared latent)
MLA_LENS = ((193, 64, 0), (257, 2, 129))
MLA_CASES = tuple((hq, dt, lq, lens) for hq, dt in ((16, F16), (128, BF16)) for lq in (1, 3) for lens in MLA_LENS)
# The MLA score is a sum over the 64 rope channels only (q is zero elsewhere): 64 ** -0.5 normalises it as D ** -0.5 normalises a D-wide
# head, so a row's visible scores have the per-key deviation of the other entries' operands (0.5 nat for q = 0.5 randn, k = randn + offset)
# and the spread over 257 keys is comparable.  The entry's default, 576 ** -0.5, would shrink the spread threefold and test less.
MLA_SM_SCALE = 64 ** -0.5

# One seed per sample (sequence), as ``ref_probe.SEEDS``: the first, in ascending order within a call, at which the reference meets the
# conditions with room -- spread <= 5.75 log2 units, smallest weight >= 2^-11.75 -- when every row sees all of the sample's keys.  Every
# mask of the tests shows a row a subset of those keys, which narrows the spread and raises the weights; the tests assert the conditions
# themselves for every mask.  Keys: ("dense", Dqk, dtype, Lq, Lk), ("varlen", Dqk, dtype), ("mla", Hq, dtype, Lq, kv_lens).
ROOM_SPREAD, ROOM_WEIGHT = 5.75, 2.0 ** -11.75
SEEDS = {
    ('dense', 256, 'f16', 200, 193): (3, 4),
    ('dense', 256, 'f16', 129, 128): (0, 1),
    ('dense', 256, 'f16', 65, 257): (2, 3),
    ('dense', 256, 'bf16', 200, 193): (1, 3),
    ('dense', 256, 'bf16', 129, 128): (0, 1),
    ('dense', 256, 'bf16', 65, 257): (2, 3),
    ('dense', 192, 'f16', 200, 193): (2, 3),
    ('dense', 192, 'f16', 129, 128): (0, 1),
    ('dense', 192, 'f16', 65, 257): (0, 2),
    ('dense', 192, 'bf16', 200, 193): (2, 3),
    ('dense', 192, 'bf16', 129, 128): (0, 1),
    ('dense', 192, 'bf16', 65, 257): (0, 2),
    ('dense', 160, 'f16', 200, 193): (2, 5),
    ('dense', 160, 'f16', 129, 128): (1, 2),
    ('dense', 160, 'f16', 65, 257): (0, 2),
    ('dense', 160, 'bf16', 200, 193): (2, 5),
    ('dense', 160, 'bf16', 129, 128): (1, 2),
    ('dense', 160, 'bf16', 65, 257): (0, 2),
    ('varlen', 192, 'f16'): (1, 2, 3, 4, 5, 6),
    ('varlen', 160, 'bf16'): (0, 1, 2, 3, 5, 6),
    ('mla', 16, 'f16', 1, (193, 64, 0)): (0, 1, 2),
    ('mla', 16, 'f16', 1, (257, 2, 129)): (0, 1, 2),
    ('mla', 16, 'f16', 3, (193, 64, 0)): (0, 1, 2),
    ('mla', 16, 'f16', 3, (257, 2, 129)): (0, 1, 2),
    ('mla', 128, 'bf16', 1, (193, 64, 0)): (0, 1, 2),
    ('mla', 128, 'bf16', 1, (257, 2, 129)): (1, 2, 3),
    ('mla', 128, 'bf16', 3, (193, 64, 0)): (2, 3, 4),
    ('mla', 128, 'bf16', 3, (257, 2, 129)): (6, 7, 8),
}


def _dt(dt):
    return "f16" if dt == F16 else "bf16"


def code(dt) -> int:
    return 0 if dt == F16 else 1


# ---------------------------------------------------------------------------------------------- operands
def dense_sample(Dqk, dt, Lq, Lk, seed):
    """q ``[HQ, Lq, Dqk]``, k ``[HKV, Lk, Dqk]`` of one sample (host): ``ref_probe.qk``."""
    q, k = rp.qk(1, HQ, HKV, Lq, Lk, Dqk, dt, seed)
    return q[0], k[0]


@functools.lru_cache(maxsize=None)
def dense_operands(Dqk, dt, Lq, Lk):
    """q ``[B, HQ, Lq, Dqk]``, k ``[B, HKV, Lk, Dqk]`` (HND, host), sample b drawn with its own seed; never modified."""
    parts = [dense_sample(Dqk, dt, Lq, Lk, s) for s in SEEDS[("dense", Dqk, _dt(dt), Lq, Lk)]]
    return torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])


@functools.lru_cache(maxsize=None)
def packed_operands(Dqk, dt):
    """Per sequence of ``SEQS`` (q ``[HQ, Lq_s, Dqk]``, k ``[HKV, Lk_s, Dqk]``), and the prefix arrays."""
    parts = [dense_sample(Dqk, dt, lq, lk, s) for (lq, lk), s in zip(SEQS, SEEDS[("varlen", Dqk, _dt(dt))])]
    cu = lambda xs: torch.tensor(np.concatenate([[0], np.cumsum(xs)]), dtype=torch.int32)
    return parts, cu([s[0] for s in SEQS]), cu([s[1] for s in SEQS])


def mla_sample(Hq, dt, Lq, n, seed):
    """q ``[Lq, Hq, 576]`` with the first 512 channels zero and ``0.5 randn`` on the rope channels; the rope channels of ``n`` latent rows
    ``[n, 64]``, ``randn`` plus a per-channel offset."""
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(Lq, Hq, 576, dtype=dt)
    q[..., 512:] = (0.5 * torch.randn(Lq, Hq, 64, generator=g)).to(dt)
    rope = (torch.randn(n, 64, generator=g) + torch.randn(1, 64, generator=g)).to(dt)
    return q, rope


@functools.lru_cache(maxsize=None)
def mla_operands(Hq, dt, Lq, lens):
    """Per sample (q ``[Lq, Hq, 576]``, rope ``[lens[b], 64]``)."""
    return [mla_sample(Hq, dt, Lq, n, s) for n, s in zip(lens, SEEDS[("mla", Hq, _dt(dt), Lq, lens)])]


def mla_kv(rope, j0, sig, dt, Lk=None, tail=0.0):
    """One sample's latent rows ``[Lk or n, 576]``: the probe of ``(j0, sig)`` on the first 512 channels, ``rope`` behind it; rows from
    ``n`` on hold ``tail``."""
    n = rope.shape[0]
    kv = torch.full((n if Lk is None else Lk, 576), tail, dtype=dt)
    kv[:n, :512] = rp.probe_v(1, n, 512, j0, [sig], dt)[0]
    kv[:n, 512:] = rope
    return kv


# ---------------------------------------------------------------------------------------------- the reference's quantised operands
def dense_aux(q, k, width, sm_scale):
    """``aux`` of one sample or sequence: q ``[Hq, Lq, D]``, k ``[Hkv, Lk, D]`` zero-padded to ``width``; per-thread INT8 with the groups
    counted from the sample's first row / key, K against its own per-channel mean (FP32 sum, rounded to the input dtype)."""
    q, k = F.pad(q, (0, width - q.shape[-1])), F.pad(k, (0, width - k.shape[-1]))
    (Hq, Lq, _), (Hkv, Lk, _) = q.shape, k.shape
    (gq, nq), (gk, nk) = ref.groups(Lq, "per_thread", "q"), ref.groups(Lk, "per_thread", "k")
    q8, qs = torch.zeros(Hq, Lq, width, dtype=torch.int8), torch.zeros(Hq, nq)
    k8, ks = torch.zeros(Hkv, Lk, width, dtype=torch.int8), torch.zeros(Hkv, nk)
    for h in range(Hkv):
        if Lk:
            k8[h], ks[h] = ref.quant_int8_per_thread(k[h], gk, nk, mean=k[h].float().mean(dim=0).to(k.dtype))
    for h in range(Hq):
        if Lq:
            q8[h], qs[h] = ref.quant_int8_per_thread(q[h], gq, nq)
    return dict(q8=q8[None], k8=k8[None], qs=qs[None], ks=ks[None], gq=gq, gk=gk, c=sm_scale * ref.LOG2E)


def mla_aux(q, kv, sm_scale):
    """``aux`` of one MLA sample: q ``[Lq, Hq, 576]`` with one scale per query row (group = position), kv ``[n, 576]`` -- the valid rows,
    probe included -- per-thread INT8 against the mean over those rows.  One kv-head."""
    Lq, Hq, _ = q.shape
    n = kv.shape[0]
    gk, nk = ref.groups(n, "per_thread", "k")
    k8, ks = ref.quant_int8_per_thread(kv, gk, nk, mean=kv.float().mean(dim=0).to(kv.dtype))
    q8, qs, own = torch.zeros(Hq, Lq, 576, dtype=torch.int8), torch.zeros(Hq, Lq), torch.arange(Hq)
    for i in range(Lq):
        q8[:, i], qs[:, i] = ref.quant_int8_per_thread(q[i], own, Hq)
    return dict(q8=q8[None], k8=k8[None, None], qs=qs[None], ks=ks[None, None], gq=torch.arange(Lq), gk=gk, c=sm_scale * ref.LOG2E)


# ---------------------------------------------------------------------------------------------- the restatement on a probe
def quant_v(v):
    """``ref_fp8_torch.quant_v_fp8`` of v ``[L, D]`` with a channel that is zero everywhere as zero bytes under a zero scale (the
    restatement divides by that abs-max; the kernels and the C oracle give ``+0`` there: tests/test_probe_host.py)."""
    v8, vs, _ = ref.quant_v_fp8(v, False)
    f = v8.float()
    f[:, vs == 0] = 0.0
    return f.to(torch.float8_e4m3fn), vs


def restate(aux, v, shift, causal, dt):
    """``ref_fp8_torch.attn_fp8`` per head on ``aux`` with v ``[Hkv, Lk, Dv]`` (zero-padded to the width of ``aux``): row i sees key j iff
    ``j <= i + shift`` (``causal``; else every key).  The diagonal is moved as tests/test_gpu_qk192_varlen.py moves it: ``shift`` zero rows
    in front of ``q8``, or its first ``-shift`` rows dropped -- a wholly masked tile is an exact no-op, so nothing else moves.  Returns
    (o float32 ``[Hq, Lq, Dv]``, lse ``[Hq, Lq]`` in log2 units); rows that see nothing are ``+0`` / ``-inf``."""
    q8, k8, qs, ks, gq, gk = aux["q8"][0], aux["k8"][0], aux["qs"][0], aux["ks"][0], aux["gq"], aux["gk"]
    (Hq, Lq, W), (Hkv, Lk, _), Dv = q8.shape, k8.shape, v.shape[-1]
    o, lse = np.zeros((Hq, Lq, Dv), dtype=np.float32), np.full((Hq, Lq), -np.inf, dtype=np.float32)
    d = shift if causal else 0
    if Lq == 0 or Lk == 0 or -d >= Lq:
        return o, lse
    sm = float(aux["c"]) / ref.LOG2E
    vq = [quant_v(F.pad(v[h], (0, W - Dv))) for h in range(Hkv)]
    first = max(-d, 0)                                              # the first row that sees a key
    for h in range(Hq):
        hk = h // (Hq // Hkv)
        q8p = torch.cat([torch.zeros(d, W, dtype=torch.int8), q8[h]]) if d >= 0 else q8[h, -d:]
        slot = torch.cat([torch.zeros(d, dtype=gq.dtype), gq]) if d >= 0 else gq[-d:]
        oo, ll = ref.attn_fp8(q8p, k8[hk], vq[hk][0], qs[h], slot, ks[hk], gk, vq[hk][1], None, causal=causal, sm_scale=sm, two_level=True,
                              out_dtype=dt)
        o[h, first:] = oo[max(d, 0):, :Dv].float().numpy()
        lse[h, first:] = ll[max(d, 0):].numpy()
    return o, lse


def restate_mla(aux, kv, dt, shift=0):
    """The restatement of tests/test_gpu_mla_decode.py on ``aux`` and the valid rows kv ``[n, 576]``: per query position i
    ``attn_fp8(causal=False)`` on the first ``n - Lq + i + 1 + shift`` keys of the already quantised K and V.  (o float32
    ``[Hq, Lq, 512]``, lse ``[Hq, Lq]``); ``+0`` / ``-inf`` for a position in front of key 0."""
    q8, k8, qs, ks, gk = aux["q8"][0], aux["k8"][0, 0], aux["qs"][0], aux["ks"][0, 0], aux["gk"]
    (Hq, Lq, _), n = q8.shape, k8.shape[0]
    o, lse = np.zeros((Hq, Lq, 512), dtype=np.float32), np.full((Hq, Lq), -np.inf, dtype=np.float32)
    if n == 0:
        return o, lse
    v8, vs = quant_v(F.pad(kv[:, :512], (0, 64)))
    sm, own = float(aux["c"]) / ref.LOG2E, torch.arange(Hq)
    for i in range(Lq):
        vis = min(n - Lq + i + 1 + shift, n)
        if vis <= 0:
            continue
        oo, ll = ref.attn_fp8(q8[:, i], k8[:vis], v8[:vis], qs[:, i], own, ks, gk[:vis], vs, None, causal=False, sm_scale=sm, two_level=True,
                              out_dtype=dt)
        o[:, i], lse[:, i] = oo[:, :512].float().numpy(), ll.numpy()
    return o, lse


# ---------------------------------------------------------------------------------------------- the engine
def conditions(aux, keep):
    """``(w_ref, spread)`` of one sample under ``keep`` with the conditions of the method asserted -- on the reference alone."""
    w, s = rp.weights_fp64(aux, keep), rp.score_spread(aux, keep)
    rp.check_conditions(w, keep, s)
    return w, s


def run_probe(what, Dv, dt, Hkv, samples, call, n_sweep):
    """``samples``: per sample (sequence) ``(n, keep [Lq_b, n], aux)`` with ``aux`` a mapping, None for a sample without keys or rows, or a
    function of the sample's signatures (the MLA entry, whose K scales see the probe; then one ``j0`` must read every key).
    ``call(j0, sig)`` runs the route on the probe of ``(j0, sig)`` and returns (per sample o ``[Hq, Lq_b, Dv]`` float32, per sample lse
    ``[Hq, Lq_b]`` or None).  First the conditions for every sample and signature, from the reference alone; then the sweeps; then
    ``ref_probe.judge`` on every sample and signature, and every key must have been read.  Returns (largest err / (bar w_ref), largest
    spread)."""
    nB = len(samples)
    sweeps = rp.sweeps(Dv, n_sweep, nB, Hkv)
    refs, spread = {}, 0.0
    for b, (n, keep, aux) in enumerate(samples):                                  # the conditions, before any output is looked at
        assert keep.shape[1] == n
        for sig in {tuple(s[b]) for _, s in sweeps}:
            if callable(aux):
                assert n_sweep <= Dv, "a reference that depends on the probe: one j0 per signature"
            a = aux(list(sig)) if callable(aux) else aux
            if a is None or n == 0 or not keep.any():
                refs[b, sig] = None
                continue
            refs[b, sig], s = conditions(a, keep)
            spread = max(spread, s)
    reads = {}
    for j0, sig in sweeps:
        os_, lses = call(j0, sig)
        for b in range(nB):
            entry = reads.setdefault((b, tuple(sig[b])), ([], []))
            entry[0].append((j0, np.asarray(os_[b], dtype=np.float32)))
            entry[1].append(None if lses is None else np.asarray(lses[b]))
    worst, known_any = 0.0, {}
    for (b, sig), (outs, lses) in reads.items():
        n, keep, _ = samples[b]
        Hq = outs[0][1].shape[0]
        w = refs[b, sig] if refs[b, sig] is not None else np.zeros((Hq,) + keep.shape)
        for lse in lses[1:]:                                                      # (the LSE does not depend on V)
            assert lse is None or np.array_equal(lse, lses[0], equal_nan=True), f"{what} sample {b}: lse differs between probe calls"
        seen, known, weights, bad = rp.read_visibility(outs, n, list(sig), Hkv)
        worst = max(worst, rp.judge(seen, known, weights, bad, keep, w, rp.BAR_F8, code(dt), lse=lses[0], what=f"{what} sample {b} sig {list(sig)}"))
        known_any[b] = known_any.get(b, False) | known
    for b, known in known_any.items():
        assert np.all(known), f"{what} sample {b}: {int((~known).sum())} keys never read"
    print(f"PROBE {what}: largest err / (bar w_ref) = {worst:.3f}, largest spread {spread:.2f} log2 units")
    return worst, spread


# ---------------------------------------------------------------------------------------------- the samples of each entry
def dense_samples(Dqk, dt, Lq, Lk, causal, width):
    """Per sample ``(Lk, keep, aux)`` of a dense call: full, or top-left causal (``j <= i``)."""
    q, k = dense_operands(Dqk, dt, Lq, Lk)
    keep = rp.visible(Lq, Lk, 0, 0, 0, causal)
    return [(Lk, keep, dense_aux(q[b], k[b], width, Dqk ** -0.5)) for b in range(B)]


def packed_keep(lq, lk, mask):
    return rp.visible(lq, lk, lk - lq if mask == "bottom_right" else 0, 0, 0, mask != "none")


def packed_samples(Dqk, dt, mask):
    """Per sequence ``(Lk_s, keep, aux)``: no mask, top-left, or bottom-right -- ``rp.visible(Lq_s, Lk_s, Lk_s - Lq_s, 0)``."""
    parts, _, _ = packed_operands(Dqk, dt)
    return [(lk, packed_keep(lq, lk, mask), dense_aux(q, k, 192, Dqk ** -0.5) if lq and lk else None) for (lq, lk), (q, k) in zip(SEQS, parts)]


def mla_keep(Lq, n):
    """Position i sees key j iff ``j < n`` and ``j <= n - Lq + i``."""
    return rp.visible(Lq, n, n - Lq, 0)


def mla_samples(Hq, dt, Lq, lens):
    """Per sample ``(kv_lens[b], keep, signature -> aux)``: the reference quantises the ``kv`` of the call, probe included."""
    ops = mla_operands(Hq, dt, Lq, lens)
    return [(n, mla_keep(Lq, n), (lambda sig, q=q, rope=rope: mla_aux(q, mla_kv(rope, 0, sig[0], dt), MLA_SM_SCALE)) if n else None)
            for n, (q, rope) in zip(lens, ops)]


# ---------------------------------------------------------------------------------------------- the seed search
def _roomy(aux, keep):
    if not keep.any():
        return True
    w = rp.weights_fp64(aux, keep)
    return rp.score_spread(aux, keep) <= ROOM_SPREAD and float(w[:, keep].min()) >= ROOM_WEIGHT


def _first(ok, start):
    s = start
    while not ok(s):
        s += 1
    return s


def find_seeds():
    """The table ``SEEDS``, searched again: per sample the first seed (behind the previous sample's) that meets the conditions with room
    when every row sees every key of the sample -- for the MLA entry under both signatures of its sweeps."""
    out = {}
    for Dqk in (256, 192, 160):
        for dt in (F16, BF16):
            for Lq, Lk in DENSE_SHAPES:
                full, seeds = np.ones((Lq, Lk), dtype=bool), []
                for b in range(B):
                    seeds.append(_first(lambda s: _roomy(dense_aux(*dense_sample(Dqk, dt, Lq, Lk, s), Dqk, Dqk ** -0.5), full), seeds[-1] + 1 if seeds else 0))
                out[("dense", Dqk, _dt(dt), Lq, Lk)] = tuple(seeds)
    for Dqk, _, dt in VARLEN_CASES:
        seeds = []
        for lq, lk in SEQS:
            ok = lambda s: not (lq and lk) or _roomy(dense_aux(*dense_sample(Dqk, dt, lq, lk, s), Dqk, Dqk ** -0.5), np.ones((lq, lk), dtype=bool))
            seeds.append(_first(ok, seeds[-1] + 1 if seeds else 0))
        out[("varlen", Dqk, _dt(dt))] = tuple(seeds)
    for Hq, dt, Lq, lens in MLA_CASES:
        seeds = []
        for b, n in enumerate(lens):
            def ok(s):
                q, rope = mla_sample(Hq, dt, Lq, n, s)
                return all(_roomy(mla_aux(q, mla_kv(rope, 0, (b + shift) % 16, dt), MLA_SM_SCALE), np.ones((Lq, n), dtype=bool)) for shift in (0, 8))
            seeds.append(_first(ok, seeds[-1] + 1 if seeds else 0) if n else (seeds[-1] + 1 if seeds else 0))
        out[("mla", Hq, _dt(dt), Lq, lens)] = tuple(seeds)
    return out


if __name__ == "__main__":
    found = find_seeds()
    print("SEEDS = {")
    for key, val in found.items():
        print(f"    {key!r}: {val!r},")
    print("}")
    print("the table in this file", "matches" if found == SEEDS else "DIFFERS")
