"""CPU: the probe-V instrument for the wide FP8-PV entries (tests/ref_probe_wide.py) pinned on the restatement, before any kernel is
judged with it (tests/test_gpu_visibility_wide.py).

  * The conditions of the method -- score spread <= 6 log2 units, every visible reference weight >= 2^-12 -- hold for every case, shape
    and mask of the GPU file, on the reference's operands alone; every seed of the table meets them with the room the table claims.  A
    case whose reference misses them fails here: nothing is skipped.
  * The restatement's own output (``ref_fp8_torch.attn_fp8`` on the probe, composed per entry as the feature files compose it) reads back
    every predicate through ``read_visibility`` and ``judge``: full, top-left, bottom-right per packed sequence, the MLA decode mask.
  * Negative controls: subtly wrong REFERENCES -- a predicate one key too wide, one key too narrow, a length off by one in either
    direction, V of the other kv-head, V of the neighbouring packed sequence, an MLA decode mask shifted by one position either way -- are
    each rejected by ``judge``.  A probe that cannot fail proves nothing; nothing here runs a kernel.
"""
import numpy as np
import pytest
import torch

import ref_probe as rp
import ref_probe_wide as rw

F16, BF16 = torch.float16, torch.bfloat16
NAME = rw._dt
MASKS = ((False, "full"), (True, "top_left"))


# ---------------------------------------------------------------------------------------------- 1. the conditions
def test_every_seed_meets_the_conditions_with_room():
    """Spread <= 5.75 and smallest weight >= 2^-11.75 when every row sees every key of the sample (MLA: under both signatures)."""
    for key, seeds in rw.SEEDS.items():
        dt = F16 if key[2] == "f16" else BF16
        if key[0] == "dense":
            _, Dqk, _, Lq, Lk = key
            for s in seeds:
                assert rw._roomy(rw.dense_aux(*rw.dense_sample(Dqk, dt, Lq, Lk, s), Dqk, Dqk ** -0.5), np.ones((Lq, Lk), dtype=bool)), (key, s)
        elif key[0] == "varlen":
            for (lq, lk), s in zip(rw.SEQS, seeds):
                if lq and lk:
                    assert rw._roomy(rw.dense_aux(*rw.dense_sample(key[1], dt, lq, lk, s), key[1], key[1] ** -0.5), np.ones((lq, lk), dtype=bool)), (key, s)
        else:
            _, Hq, _, Lq, lens = key
            for b, (n, s) in enumerate(zip(lens, seeds)):
                q, rope = rw.mla_sample(Hq, dt, Lq, n, s)
                for shift in (0, 8):
                    assert not n or rw._roomy(rw.mla_aux(q, rw.mla_kv(rope, 0, (b + shift) % 16, dt), rw.MLA_SM_SCALE), np.ones((Lq, n), dtype=bool)), (key, s)
    assert len(rw.SEEDS) == 18 + len(rw.VARLEN_CASES) + len(rw.MLA_CASES)


def _report(what, found):
    spread = max((s for _, s, _ in found), default=0.0)
    least = min((l for _, _, l in found), default=1.0)
    print(f"{what}: {len(found)} samples, largest spread {spread:.2f} log2 units, smallest visible weight 2^{np.log2(least):.2f}")


def _conditions(samples, sigs=((0,),)):
    out = []
    for b, (n, keep, aux) in enumerate(samples):
        for sig in sigs:
            a = aux([(b + sig[0]) % 16]) if callable(aux) else aux
            if a is None or not keep.any():
                continue
            w, s = rw.conditions(a, keep)
            out.append((b, s, float(w[:, keep].min())))
    return out


def test_conditions_hold_for_every_dense_case_shape_and_mask():
    found = []
    for Dqk, dt, width in [(d, dt, 256) for d, dt, _ in rw.HD256_CASES] + [(d, dt, 192) for d, _, dt, _ in rw.QK192_CASES]:
        for Lq, Lk in rw.DENSE_SHAPES:
            for causal, _ in MASKS:
                found += _conditions(rw.dense_samples(Dqk, dt, Lq, Lk, causal, width))
    assert len(found) == 8 * 3 * 2 * rw.B
    _report("dense", found)


def test_conditions_hold_for_every_packed_case_and_mask():
    found = []
    for Dqk, _, dt in rw.VARLEN_CASES:
        for mask in rw.VARLEN_MASKS:
            found += _conditions(rw.packed_samples(Dqk, dt, mask))
    assert len(found) == len(rw.VARLEN_CASES) * 3 * 4              # (four of the six sequences have rows and keys)
    _report("packed", found)


def test_conditions_hold_for_every_mla_case_under_both_signatures():
    found = []
    for Hq, dt, Lq, lens in rw.MLA_CASES:
        found += _conditions(rw.mla_samples(Hq, dt, Lq, lens), sigs=((0,), (8,)))
    _report("mla", found)
    assert found


# ---------------------------------------------------------------------------------------------- 2. the instrument on the restatement
def _dense_call(samples, Dv, dt, causal, shift=0, v_map=lambda v: v, auxes=None, n_probe=None):
    """``call`` of the engine: the restatement on every sample of ``samples`` (``auxes``: the operands it believes in, default the
    samples' own; ``n_probe``: rows of the probe, default the sample's length)."""
    def call(j0, sig):
        outs = [rw.restate(aux if auxes is None else auxes[b], v_map(rp.probe_v(rw.HKV, n_probe or n, Dv, j0, sig[b], dt)), shift, causal, dt)
                for b, (n, _, aux) in enumerate(samples)]
        return [o for o, _ in outs], [l for _, l in outs]
    return call


@pytest.mark.parametrize("causal,mask", MASKS, ids=[m for _, m in MASKS])
@pytest.mark.parametrize("Lq,Lk", rw.DENSE_SHAPES, ids=[f"{a}x{b}" for a, b in rw.DENSE_SHAPES])
@pytest.mark.parametrize("Dqk,Dv,dt,width", [(256, 256, F16, 256), (192, 192, BF16, 256), (192, 128, BF16, 192), (160, 64, F16, 192)],
                         ids=["hd256-d256-f16", "hd256-d192-bf16", "qk192-192v128-bf16", "qk192-160v64-f16"])
def test_restatement_reads_back_the_dense_predicates(Dqk, Dv, dt, width, Lq, Lk, causal, mask):
    """Sample 0 of each dense case (the samples differ in their seed only)."""
    samples = rw.dense_samples(Dqk, dt, Lq, Lk, causal, width)[:1]
    worst, _ = rw.run_probe(f"restatement {Dqk}/{Dv} {Lq}x{Lk} {mask}", Dv, dt, rw.HKV, samples, _dense_call(samples, Dv, dt, causal), Lk)
    assert worst <= 1.0


def _packed_call(samples, seqs, Dv, dt, mask, v_of=lambda b: b):
    """``call`` for packed sequences ``seqs`` ``[(Lq_s, Lk_s)]``: sequence b reads the V rows of sequence ``v_of(b)``'s probe (its own
    key count of them, zero rows behind a shorter neighbour)."""
    def call(j0, sig):
        outs = []
        for b, ((lq, lk), (n, _, aux)) in enumerate(zip(seqs, samples)):
            src = v_of(b)
            v = torch.zeros(rw.HKV, lk, Dv, dtype=dt)
            take = min(lk, seqs[src][1])
            v[:, :take] = rp.probe_v(rw.HKV, seqs[src][1], Dv, j0, sig[src], dt)[:, :take]
            if aux is None:
                outs.append((np.zeros((rw.HQ, lq, Dv), dtype=np.float32), np.full((rw.HQ, lq), -np.inf, dtype=np.float32)))
            else:
                outs.append(rw.restate(aux, v, lk - lq if mask == "bottom_right" else 0, mask != "none", dt))
        return [o for o, _ in outs], [l for _, l in outs]
    return call


@pytest.mark.parametrize("mask", rw.VARLEN_MASKS)
def test_restatement_reads_back_the_packed_predicates(mask):
    Dqk, Dv, dt = rw.VARLEN_CASES[0]
    samples = rw.packed_samples(Dqk, dt, mask)
    worst, _ = rw.run_probe(f"restatement packed {mask}", Dv, dt, rw.HKV, samples, _packed_call(samples, rw.SEQS, Dv, dt, mask), max(s[1] for s in rw.SEQS))
    assert worst <= 1.0


def _mla_call(ops, dt, shift=0):
    def call(j0, sig):
        outs = []
        for b, (q, rope) in enumerate(ops):
            if rope.shape[0] == 0:                                  # a sample without keys: +0 / -inf by contract
                outs.append((np.zeros((q.shape[1], q.shape[0], 512), dtype=np.float32), np.full((q.shape[1], q.shape[0]), -np.inf, dtype=np.float32)))
                continue
            kv = rw.mla_kv(rope, j0, sig[b][0], dt)
            outs.append(rw.restate_mla(rw.mla_aux(q, kv, rw.MLA_SM_SCALE), kv, dt, shift))
        return [o for o, _ in outs], [l for _, l in outs]
    return call


MLA_HOST = [c for c in rw.MLA_CASES if c[0] == 16 or (c[2], c[3]) == (3, rw.MLA_LENS[1])]


@pytest.mark.parametrize("Hq,dt,Lq,lens", MLA_HOST, ids=[f"h{h}-{NAME(dt)}-q{lq}-{'_'.join(map(str, lens))}" for h, dt, lq, lens in MLA_HOST])
def test_restatement_reads_back_the_mla_decode_mask(Hq, dt, Lq, lens):
    """Every Hq 16 case, and Hq 128 at Lq 3 with a sample of two keys (a position in front of key 0)."""
    worst, _ = rw.run_probe(f"restatement mla h{Hq} q{Lq} {lens}", 512, dt, 1, rw.mla_samples(Hq, dt, Lq, lens),
                            _mla_call(rw.mla_operands(Hq, dt, Lq, lens), dt), max(lens))
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------- 3. negative controls on the reference
def _rejected(*probe_args):
    """True iff the engine's assertions reject the (wrong) reference behind ``call`` when it is held to the right predicate."""
    try:
        rw.run_probe(*probe_args)
    except AssertionError as e:
        print("reported:", str(e)[:200])
        return True
    return False


C_D, C_DT, C_LQ, C_LK = 256, F16, 129, 128        # the dense control setup: hd256's width, the diagonal ending on a tile boundary


def _control(causal=True):
    return rw.dense_samples(C_D, C_DT, C_LQ, C_LK, causal, 256)[:1]


def _dense_rejected(samples, call, n_sweep=C_LK):
    return _rejected("control", C_D, C_DT, rw.HKV, samples, call, n_sweep)


def test_the_right_references_pass_the_control_setups():
    s = _control()
    assert not _dense_rejected(s, _dense_call(s, C_D, C_DT, True))
    s = _control(False)
    assert not _dense_rejected(s, _dense_call(s, C_D, C_DT, False))


def test_control_predicate_one_key_too_wide():
    s = _control()
    assert _dense_rejected(s, _dense_call(s, C_D, C_DT, True, shift=1))


def test_control_predicate_one_key_too_narrow():
    s = _control()
    assert _dense_rejected(s, _dense_call(s, C_D, C_DT, True, shift=-1))


def test_control_v_of_the_other_kv_head():
    s = _control(False)
    assert _dense_rejected(s, _dense_call(s, C_D, C_DT, False, v_map=lambda v: v[[1, 1]]))


def test_control_length_off_by_one():
    """A reference that believes the sample one key shorter (its operands and V rows end at key 126), and one that believes it one key
    longer: the true length is 127, the probe carries on behind it, and the reference reads key 127."""
    s = _control(False)
    q, k = rw.dense_operands(C_D, C_DT, C_LQ, C_LK)
    short = rw.dense_aux(q[0], k[0, :, :C_LK - 1], 256, C_D ** -0.5)
    assert _dense_rejected(s, _dense_call(s, C_D, C_DT, False, v_map=lambda v: v[:, :C_LK - 1], auxes=[short]))
    truth = [(C_LK - 1, s[0][1][:, :C_LK - 1], short)]
    assert not _dense_rejected(truth, _dense_call(truth, C_D, C_DT, False))
    assert _dense_rejected(truth, _dense_call(truth, C_D, C_DT, False, auxes=[s[0][2]], n_probe=C_LK))


@pytest.mark.parametrize("mask", ["none", "bottom_right"])
def test_control_v_of_the_neighbouring_packed_sequence(mask):
    """Sequences (64, 64) and (72, 200) of the packed batch: the second reads the first 64 V rows of the first one's probe (keys 0 .. 63 at
    the same positions, the neighbour's signature and length), as a V tile base one sequence off would."""
    Dqk, Dv, dt = rw.VARLEN_CASES[0]
    seqs, samples = rw.SEQS[2:4], rw.packed_samples(Dqk, dt, mask)[2:4]
    assert not _rejected("control", Dv, dt, rw.HKV, samples, _packed_call(samples, seqs, Dv, dt, mask), 200)
    assert _rejected("control", Dv, dt, rw.HKV, samples, _packed_call(samples, seqs, Dv, dt, mask, v_of=lambda b: 0), 200)


@pytest.mark.parametrize("shift", [1, -1])
def test_control_mla_decode_mask_shifted_by_one_position(shift):
    Hq, dt, Lq, lens = 16, F16, 3, rw.MLA_LENS[0]
    samples, ops = rw.mla_samples(Hq, dt, Lq, lens)[1:2], rw.mla_operands(Hq, dt, Lq, lens)[1:2]
    # (alone in its call the sample carries signature 0; its seed met the conditions under 1 and 9: the engine asserts them again)
    assert not _rejected("control", 512, dt, 1, samples, _mla_call(ops, dt), 64)
    assert _rejected("control", 512, dt, 1, samples, _mla_call(ops, dt, shift=shift), 64)
