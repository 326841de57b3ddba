"""CPU: the probe-V instrument (tests/ref_probe.py) pinned on the references, before any kernel is judged with it.

  * On ``ref_window.attn_window`` (the FP8-PV arithmetic with a visibility predicate, on the oracle's quantised operands) and on the C
    oracle's own causal path: the visibility set is read back exactly, every weight lies within the derived FP8 bar of the FP64 softmax,
    a zero channel reads ``+0``.
  * The conditions of the method -- score spread <= 6 log2 units, every visible reference weight >= 2^-12 -- hold for every (D, dtype) and
    every mask of tests/test_gpu_visibility.py's dense calls, on the reference's operands alone.
  * Negative controls: five subtly wrong REFERENCES (a predicate one key too wide on the right, one key too narrow on the left, two
    64-key blocks of keys swapped, the other kv-head's V, a length off by one) are each reported by the decoder.  This is the evidence
    that the GPU tests would fail on a kernel that wrong; nothing here runs a kernel.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_probe as rp
import ref_window as rw
import util

F16 = torch.float16


@functools.lru_cache(maxsize=None)
def _operands(D, dt):
    return rp.operands(D, dt)


def _aux(oracle, q, k, code, causal=True):
    """The oracle's quantised operands of one sample (q ``[1, Hq, Lq, D]``, k ``[1, Hkv, n, D]``): per-thread INT8 Q / K, K smoothed."""
    _, _, aux = oracle.sageattn_dense(util.bits(q), util.bits(k), util.bits(torch.zeros_like(k)), code, is_causal=causal, pv="f8",
                                      qk_quant_gran="per_thread", fp8_scores="exact")
    return aux


def _restatement(oracle, aux, code, dt, D, keep, v):
    """``attn_window`` on the oracle's operands with the probe ``v`` ``[Hkv, n, D]``: (o float32 ``[Hq, Lq, D]``, lse)."""
    vp = F.pad(v[None], (0, aux["q8"].shape[-1] - D))
    v8, vs = oracle.quant_v_fp8(util.bits(vp), code)
    o, lse = rw.attn_window(aux["q8"][0], aux["k8"][0], v8[0], aux["qs"][0], aux["gq"], aux["ks"][0], aux["gk"], vs[0], keep,
                            c=np.float32(aux["c"]), out_dtype=dt)
    return o.float().numpy()[..., :D], lse.numpy()


def _sweep(n, D, run, shifts=(0, 8)):
    """Both sweeps of one sample through ``run(v) -> (o, lse)``: ``[(sig, [(j0, o)], lse)]``."""
    by_sig = {}
    for j0, sig in rp.sweeps(D, n, 1, rp.HKV):
        if (sig[0][0] - 0) % 16 not in shifts:
            continue
        o, lse = run(rp.probe_v(rp.HKV, n, D, j0, sig[0], run.dtype))
        by_sig.setdefault(tuple(sig[0]), ([], []))
        by_sig[tuple(sig[0])][0].append((j0, o))
        by_sig[tuple(sig[0])][1].append(lse)
    return [(list(sig), outs, lses[0]) for sig, (outs, lses) in by_sig.items()]


def _judge_sample(n, D, code, run, keep, w_ref, what, shifts=(0, 8)):
    """Decode and judge both sweeps; every key must have been read by one of them.  Returns the largest weight-error ratio."""
    worst, known_any = 0.0, np.zeros((rp.HQ, n), dtype=bool)
    for sig, outs, lse in _sweep(n, D, run, shifts):
        seen, known, weights, bad = rp.read_visibility(outs, n, sig, rp.HKV)
        worst = max(worst, rp.judge(seen, known, weights, bad, keep, w_ref, rp.BAR_F8, code, lse=lse, what=f"{what} sig {sig}"))
        known_any |= known
    assert known_any.all() or len(shifts) < 2, f"{what}: {int((~known_any).sum())} keys never read"
    return worst


# ---------------------------------------------------------------------------------------------- 1. the conditions, every dense mask
@pytest.mark.parametrize("case", rp.CASES, ids=rp.CASE_IDS)
def test_conditions_hold_for_every_dense_mask(oracle_mod, case):
    D, dt, _ = case
    code = 0 if dt == F16 else 1
    q, k = _operands(D, dt)
    worst_spread, least = 0.0, 1.0
    aux_of = functools.lru_cache(maxsize=None)(lambda b, n: _aux(oracle_mod, q[b:b + 1], k[b:b + 1, :, :n].contiguous(), code))
    masks = dict(rp.dense_masks())
    masks["plain"] = [(n, 0, 0, 0, c) for n in (rp.LK, 257) for c in (False, True)]      # (samples 0 and 1 of the batch)
    for name, batch in masks.items():
        for b, (n, s, W, r, causal) in enumerate(batch):
            b = b % 2 if name == "plain" else b
            if n == 0:
                continue
            keep = rp.visible(rp.LQ, n, s, W, r, causal)
            aux = aux_of(b, n)
            w, spread = rp.weights_fp64(aux, keep), rp.score_spread(aux, keep)
            rp.check_conditions(w, keep, spread)
            worst_spread = max(worst_spread, spread)
            if keep.any():
                least = min(least, float(w[:, keep].min()))
    print(f"{rp.CASE_IDS[rp.CASES.index(case)]}: largest spread {worst_spread:.2f} log2 units, smallest visible weight 2^{np.log2(least):.2f}")


# ---------------------------------------------------------------------------------------------- 2. the instrument on the restatement
@pytest.mark.parametrize("case", rp.CASES, ids=rp.CASE_IDS)
def test_restatement_reads_back_every_triple(oracle_mod, case):
    """Every (len, q_start, W) triple of the GPU file, each on the sample of the batch that carries it, and the two non-causal windows."""
    D, dt, _ = case
    code = 0 if dt == F16 else 1
    q, k = _operands(D, dt)
    cases = [(t % 6, n, s, W, 0) for t, (n, s, W) in enumerate(rp.TRIPLES)] + [(3, 193, 130, 131, 30), (2, 257, 57, 0, 30)]
    worst = 0.0
    for b, n, s, W, r in cases:
        keep = rp.visible(rp.LQ, n, s, W, r)
        if n == 0:                                               # nothing to attend to: the predicate's rows are all empty
            assert not keep.any()
            continue
        aux = _aux(oracle_mod, q[b:b + 1], k[b:b + 1, :, :n].contiguous(), code)
        w = rp.weights_fp64(aux, keep)
        rp.check_conditions(w, keep, rp.score_spread(aux, keep))
        run = lambda v: _restatement(oracle_mod, aux, code, dt, D, keep, v)
        run.dtype = dt
        worst = max(worst, _judge_sample(n, D, code, run, keep, w, f"len {n} offset {s} window {W} shift {r}"))
    print(f"restatement, {rp.CASE_IDS[rp.CASES.index(case)]}: largest err / (bar w_ref) = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("case", rp.CASES[:2], ids=rp.CASE_IDS[:2])
def test_oracle_causal_path_reads_back(oracle_mod, case):
    """The C oracle's own FP8 path with the predicates it can express: non-causal, and top-left causal on a square call."""
    D, dt, _ = case
    code = 0 if dt == F16 else 1
    q, k = _operands(D, dt)
    n = rp.LQ
    qb, kb = q[:1], k[:1, :, :n].contiguous()
    for causal in (False, True):
        keep = rp.visible(rp.LQ, n, 0, 0, 0, causal)

        def run(v):
            o, lse, _ = oracle_mod.sageattn_dense(util.bits(qb), util.bits(kb), util.bits(v[None]), code, is_causal=causal, pv="f8",
                                                  qk_quant_gran="per_thread", fp8_scores="exact", return_lse=True)
            return util.f32(o, code)[0], lse[0]
        run.dtype = dt
        aux = _aux(oracle_mod, qb, kb, code, causal)
        w = rp.weights_fp64(aux, keep)
        rp.check_conditions(w, keep, rp.score_spread(aux, keep))
        _judge_sample(n, D, code, run, keep, w, f"oracle causal={causal}")


def test_a_zero_channel_reads_plus_zero(oracle_mod):
    """The corner the probe rests on: a V channel that is zero everywhere (abs-max 0) gives ``+0`` in every row, on the oracle and on the
    restatement -- not NaN, not ``-0``."""
    D, dt, code = 64, F16, 0
    q, k = _operands(D, dt)
    n = 130
    qb, kb = q[:1], k[:1, :, :n].contiguous()
    v = torch.zeros(rp.HKV, n, D, dtype=dt)
    v[:, :, 1::2] = torch.randn(rp.HKV, n, D // 2, generator=torch.Generator().manual_seed(3)).to(dt)
    o, _, aux = oracle_mod.sageattn_dense(util.bits(qb), util.bits(kb), util.bits(v[None]), code, is_causal=True, pv="f8",
                                          qk_quant_gran="per_thread", fp8_scores="exact")
    o2, _ = _restatement(oracle_mod, aux, code, dt, D, rp.visible(rp.LQ, n, 0, 0), v)
    for got in (util.f32(o, code)[0], o2):
        assert not got[..., 0::2].any() and not np.signbit(got[..., 0::2]).any()
        assert np.isfinite(got).all() and got[..., 1::2].any()


# ---------------------------------------------------------------------------------------------- 3. negative controls on the reference
LQ_NEG, N_NEG, S_NEG, W_NEG = 70, 193, 130, 37


@functools.lru_cache(maxsize=None)
def _neg_setup():
    import oracle
    oracle.build()
    D, dt, code = 64, F16, 0
    q, k = _operands(D, dt)
    qb, kb = q[3:4, :, :LQ_NEG].contiguous(), k[3:4, :, :N_NEG].contiguous()
    aux = _aux(oracle, qb, kb, code)
    keep = rp.visible(LQ_NEG, N_NEG, S_NEG, W_NEG)
    return oracle, aux, keep, rp.weights_fp64(aux, keep)


def _reported(run_wrong, n_read=N_NEG):
    """True iff the decoder's assertions reject the (wrong) reference ``run_wrong`` when held to the right predicate."""
    oracle, aux, keep, w = _neg_setup()
    run_wrong.dtype = F16
    try:
        _judge_sample(n_read, 64, 0, run_wrong, keep[:, :n_read], w[:, :, :n_read], "negative control")
    except AssertionError as e:
        print("reported:", str(e)[:160])
        return True
    return False


def _run_with(keep_used, v_map=lambda v: v):
    oracle, aux, _, _ = _neg_setup()
    return lambda v: _restatement(oracle, aux, 0, F16, 64, keep_used, v_map(v))


def test_the_right_reference_passes_the_control_setup():
    _, _, keep, _ = _neg_setup()
    assert not _reported(_run_with(keep))


def test_control_predicate_one_key_too_wide_on_the_right():
    assert _reported(_run_with(rp.visible(LQ_NEG, N_NEG, S_NEG + 1, W_NEG + 1)))


def test_control_predicate_one_key_too_narrow_on_the_left():
    assert _reported(_run_with(rp.visible(LQ_NEG, N_NEG, S_NEG, W_NEG - 1)))


def test_control_two_key_blocks_swapped():
    """Keys 64..127 taken for 128..191 and back: each weight shows up under the other block's key."""
    _, _, keep, _ = _neg_setup()
    perm = torch.arange(N_NEG)
    perm[64:128], perm[128:192] = torch.arange(128, 192), torch.arange(64, 128)
    assert _reported(_run_with(keep, lambda v: v[:, perm]))


def test_control_v_of_the_other_kv_head():
    _, _, keep, _ = _neg_setup()
    assert _reported(_run_with(keep, lambda v: v[[1, 1]]))


def test_control_length_off_by_one():
    """A reference that believes the sample one key shorter, and one that believes it one key longer (reading one more V row than the
    probe of the true length has a channel for: the decoder is given the longer sweep and the true predicate padded with a dark key)."""
    oracle, aux, keep, w = _neg_setup()
    short = keep.copy()
    short[:, N_NEG - 1] = False
    assert _reported(_run_with(short))
    # one key longer: the operands of n + 1 keys under the causal window of n + 1, judged by the predicate of n keys
    D, dt, code = 64, F16, 0
    q, k = _operands(D, dt)
    qb, kb = q[3:4, :, :LQ_NEG].contiguous(), k[3:4, :, :N_NEG + 1].contiguous()
    aux1 = _aux(oracle, qb, kb, code)
    keep1 = rp.visible(LQ_NEG, N_NEG + 1, S_NEG, W_NEG)
    assert keep1[:, N_NEG].any()                                                       # (the extra key is one some row would see)
    run = lambda v: _restatement(oracle, aux1, code, dt, D, keep1, v)
    run.dtype = dt
    dark = np.concatenate([keep, np.zeros((LQ_NEG, 1), dtype=bool)], axis=1)
    wd = np.concatenate([w, np.zeros((rp.HQ, LQ_NEG, 1))], axis=2)
    try:
        _judge_sample(N_NEG + 1, D, code, run, dark, wd, "one key longer")
    except AssertionError as e:
        print("reported:", str(e)[:160])
    else:
        raise AssertionError("a sample one key too long was not reported")
