"""GPU: WHICH KEYS each row attended to, read exactly through probe values of V (tests/ref_probe.py), on the wide FP8-PV entries:
``hd256.sageattn_hd256``, ``qk192.sageattn_qk192``, ``qk192_varlen.sageattn_qk192_varlen`` and ``mla_decode.sageattn_mla_decode``.

Their feature files hold random data to ``2e-3 max|o|``; an off-by-one at a mask edge, or a V tile of another kv-head or sequence, is not
forced above that bar when V is i.i.d. over 200 to 449 keys.  Here channel ``d`` of V holds a single 1.0 in the row of key ``j0 + d``, so
``o[i, d]`` is the weight of row ``i`` on that key and ``+0`` iff the key is invisible; the signature holes (one set per (sample, kv-head)
or (sequence, kv-head)) must read ``+0``.  tests/test_gpu_visibility.py does this for D 64, 96 and 128; tests/ref_probe_wide.py holds what
the wide entries need on top (their reference operands at the padded width, the MLA entry's V made a free operand by ``q[..., :512] =
0``), and tests/test_probe_wide_host.py pins it on the restatement and shows that subtly wrong references are rejected.

Assertions per sample and sweep, ``ref_probe.judge`` in its fixed order: exact visibility on every key read; no violation; ``lse = -inf``
exactly in the predicate's empty rows; row sums; per-key weights within ``ref_probe.BAR_F8 * w_ref`` plus one output ulp.  The conditions
of the method (``ref_probe.MAX_SPREAD``, ``ref_probe.MIN_WEIGHT``) are asserted on the reference alone before an output is looked at; a
case whose reference misses them fails.

Shapes: dense B 2, Hq 4, Hkv 2, (Lq, Lk) in (200, 193), (129, 128), (65, 257) -- the top-left diagonal's end and the last key one after,
on and one before a 64-key boundary; packed: six sequences with a bottom-right shift of 63 and of -128, one without rows, one without keys;
MLA: B 3, Hq 16 / 128, Lq 1 / 3, ``kv_lens`` (193, 64, 0) / (257, 2, 129), rows past a sample's length NaN.

Measured on an MI355X -- per entry the largest ``err / (bar * w_ref)`` of any case (each test prints its own) and the largest score
spread of its cases in log2 units.  No entry failed the set equality or a bar.

    entry                                                      ratio   spread
    sageattn_hd256, D 256 / 192, full / top-left               0.929   5.73
    sageattn_qk192, 192 / 128 and 160 / 64, full / top-left    0.929   5.71
    sageattn_qk192_varlen, none / top-left / bottom-right      0.924   5.74
    sageattn_mla_decode, Hq 16 / 128, Lq 1 / 3                 0.924   5.73

The ratios are e4m3's half ulp over the bar (fp16 outputs read 0.88, bf16 outputs 0.92 - 0.93), as on the D <= 128 routes; the
restatement itself reads the same on the CPU (tests/test_probe_wide_host.py).
"""
import numpy as np
import pytest
import torch

import ref_probe as rp
import ref_probe_wide as rw

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DEV = torch.device("cuda:0")
NAME = lambda dt: "f16" if dt == F16 else "bf16"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lay(t, layout):
    return t if layout == "HND" else t.transpose(1, 2).contiguous()


def _host(o, layout):
    """A device output in ``layout`` as float32 numpy, HND."""
    return (o if layout == "HND" else o.transpose(1, 2)).float().cpu().numpy()


def _dense_call(fn, Dqk, Dv, dt, layout, Lq, Lk, causal):
    q, k = rw.dense_operands(Dqk, dt, Lq, Lk)
    qd, kd = _lay(q.to(DEV), layout), _lay(k.to(DEV), layout)

    def call(j0, sig):
        v = torch.stack([rp.probe_v(rw.HKV, Lk, Dv, j0, sig[b], dt) for b in range(rw.B)])
        o, lse = fn(qd, kd, _lay(v.to(DEV), layout), tensor_layout=layout, is_causal=causal, return_lse=True)
        assert o.shape[-1] == Dv
        return _host(o, layout), lse.cpu().numpy()
    return call


# ---------------------------------------------------------------------------------------------- 1. sageattn_hd256
@pytest.mark.parametrize("causal", [False, True], ids=["full", "top_left"])
@pytest.mark.parametrize("Lq,Lk", rw.DENSE_SHAPES, ids=[f"{a}x{b}" for a, b in rw.DENSE_SHAPES])
@pytest.mark.parametrize("case", rw.HD256_CASES, ids=[f"d{d}-{NAME(dt)}-{lay}" for d, dt, lay in rw.HD256_CASES])
def test_hd256(case, Lq, Lk, causal):
    """D 256 (read in place) and D 192 (behind ``F.pad``): the probe has D channels, so one ``j0`` call reads up to 240 keys."""
    from sageattention_amd.hd256 import sageattn_hd256
    D, dt, layout = case
    samples = rw.dense_samples(D, dt, Lq, Lk, causal, 256)
    rw.run_probe(f"hd256 d{D} {Lq}x{Lk} {'top_left' if causal else 'full'}", D, dt, rw.HKV, samples,
                 _dense_call(sageattn_hd256, D, D, dt, layout, Lq, Lk, causal), Lk)


# ---------------------------------------------------------------------------------------------- 2. sageattn_qk192
@pytest.mark.parametrize("causal", [False, True], ids=["full", "top_left"])
@pytest.mark.parametrize("Lq,Lk", rw.DENSE_SHAPES, ids=[f"{a}x{b}" for a, b in rw.DENSE_SHAPES])
@pytest.mark.parametrize("case", rw.QK192_CASES, ids=[f"d{a}v{b}-{NAME(dt)}-{lay}" for a, b, dt, lay in rw.QK192_CASES])
def test_qk192(case, Lq, Lk, causal):
    """192 / 128, and 160 / 64 where the probe has 64 channels (both operands padded by the entry)."""
    from sageattention_amd.qk192 import sageattn_qk192
    Dqk, Dv, dt, layout = case
    samples = rw.dense_samples(Dqk, dt, Lq, Lk, causal, 192)
    rw.run_probe(f"qk192 {Dqk}/{Dv} {Lq}x{Lk} {'top_left' if causal else 'full'}", Dv, dt, rw.HKV, samples,
                 _dense_call(sageattn_qk192, Dqk, Dv, dt, layout, Lq, Lk, causal), Lk)


# ---------------------------------------------------------------------------------------------- 3. sageattn_qk192_varlen
VARLEN_KW = {"none": dict(is_causal=False, causal_align="top_left"), "top_left": dict(is_causal=True, causal_align="top_left"),
             "bottom_right": dict(is_causal=True, causal_align="bottom_right")}


@pytest.mark.parametrize("mask", rw.VARLEN_MASKS)
@pytest.mark.parametrize("case", rw.VARLEN_CASES, ids=[f"d{a}v{b}-{NAME(dt)}" for a, b, dt in rw.VARLEN_CASES])
def test_qk192_varlen(case, mask):
    """Six packed sequences, one signature per (sequence, kv-head), key positions counted from the sequence's own first key: a V tile of
    the neighbouring sequence or of the other kv-head shows as a weight in a hole, or as a hole where a weight belongs."""
    from sageattention_amd.qk192_varlen import sageattn_qk192_varlen
    Dqk, Dv, dt = case
    parts, cu_q, cu_k = rw.packed_operands(Dqk, dt)
    qd = torch.cat([q.transpose(0, 1) for q, _ in parts]).contiguous().to(DEV)
    kd = torch.cat([k.transpose(0, 1) for _, k in parts]).contiguous().to(DEV)
    cq, ck = cu_q.to(DEV), cu_k.to(DEV)
    mq, mk = max(s[0] for s in rw.SEQS), max(s[1] for s in rw.SEQS)
    cut = lambda t, b: t[:, int(cu_q[b]):int(cu_q[b + 1])]

    def call(j0, sig):
        v = rp.probe_v_packed(rw.HKV, cu_k, Dv, j0, sig, dt)
        o, lse = sageattn_qk192_varlen(qd, kd, v.to(DEV), cq, ck, mq, mk, return_lse=True, **VARLEN_KW[mask])
        assert o.shape == (qd.shape[0], rw.HQ, Dv)
        o, lse = o.float().cpu().numpy().transpose(1, 0, 2), lse.cpu().numpy()
        return [np.ascontiguousarray(cut(o, b)) for b in range(len(rw.SEQS))], [cut(lse, b) for b in range(len(rw.SEQS))]

    rw.run_probe(f"qk192_varlen {Dqk}/{Dv} {mask}", Dv, dt, rw.HKV, rw.packed_samples(Dqk, dt, mask), call, mk)


# ---------------------------------------------------------------------------------------------- 4. sageattn_mla_decode
@pytest.mark.parametrize("Hq,dt,Lq,lens", rw.MLA_CASES, ids=[f"h{h}-{NAME(dt)}-q{lq}-{'_'.join(map(str, lens))}" for h, dt, lq, lens in rw.MLA_CASES])
def test_mla_decode(Hq, dt, Lq, lens):
    """``q[..., :512] = 0`` makes V = ``kv[..., :512]`` a free operand (tests/ref_probe_wide.py); 512 channels read every key in one call.
    Signatures are per sample; rows of ``kv`` from ``kv_lens[b]`` on hold NaN.  The predicate: ``j < kv_lens[b]`` and
    ``j <= kv_lens[b] - Lq + i``."""
    from sageattention_amd.mla_decode import sageattn_mla_decode
    ops, Lk = rw.mla_operands(Hq, dt, Lq, lens), max(lens)
    qd = torch.stack([q for q, _ in ops]).to(DEV)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)

    def call(j0, sig):
        kv = torch.stack([rw.mla_kv(rope, j0, sig[b][0], dt, Lk=Lk, tail=float("nan")) for b, (_, rope) in enumerate(ops)])
        o, lse = sageattn_mla_decode(qd, kv.to(DEV), lens_dev, sm_scale=rw.MLA_SM_SCALE, return_lse=True)
        assert o.shape == (len(lens), Lq, Hq, 512) and lse.shape == (len(lens), Hq, Lq)
        return o.float().cpu().numpy().transpose(0, 2, 1, 3), lse.cpu().numpy()

    rw.run_probe(f"mla_decode h{Hq} q{Lq} lens {lens}", 512, dt, 1, rw.mla_samples(Hq, dt, Lq, lens), call, Lk)
