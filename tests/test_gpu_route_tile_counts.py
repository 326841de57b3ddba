"""GPU: tile-count sweeps of the FP8-PV units behind ``kv_lens`` (``*_f8k``), ``q_start`` (``*_f8q``), ``window_size`` (``*_f8w``), ``pack_gqa``
(``*_f8g``) and the packed bottom-right / window launches (``*_f8vb``, ``*_f8vbw``).

Every one of these units compiles the hand-scheduled pipelined loop (csrc/sage_attn_loop_f8.h) on its own: six bodies per trip, a remainder of
up to five bodies renamed behind them, the last-tile bodies.  The feature tests run them at Lk = 640 -- at most eight tiles, never a second trip,
never a remainder behind a trip.  Here the keys are padded to 1536 (24 tiles) and the lengths, offsets and windows are CHOSEN with
tests/loop_plan.py, the host model of a work item's loop partition, so that every unit runs 0, 1 and 2 trips with every remainder 0 .. 5, behind
0 .. 3 head tiles where it has them, with and without the last-tile bodies.  What the selections reach is asserted in
tests/test_loop_plan_host.py (on the CPU, next to the check of the model itself); every case prints the model's forms next to its distance.

References, each the existing test's own for the route, none looser:
  a. kv_lens: each sample equals, bit for bit, the plain call on its first len_b keys (test_gpu_kv_lens.py);
  b. q_start: multiples of 128 equal the padded plain call bit for bit (test_gpu_q_start.py); every other offset against
     ``ref_window.attn_window`` under ``visible(W=0)`` on the oracle's quantised operands, bar ``2e-3 max|ref| + 2 output ulps``, LSE within 5e-3,
     rows without keys exactly +0 / -inf and the predicate's rows (test_gpu_window.py::_check);
  c. window_size: the same reference and bar (test_gpu_window.py::_check);
  d. pack_gqa: the packed call equals the unpacked call bit for bit, and the grid probe confirms the packed launch (test_gpu_gqa_pack.py);
  e. packed bottom-right / window: ``ref_varlen_br`` / ``ref_varlen_window`` at those files' bars (test_gpu_varlen_br.py: one output ulp;
     test_gpu_varlen_window.py: two), and the ticket launch equals the ordinary one bit for bit.

Shapes: Hq = 2, Hkv = 1 (pack_gqa: groups of 4 and 5), D in {128, 64}, Lq = 200 -- one whole and one ragged query block -- except the causal
top-left kv_lens sweep, where the diagonal caps the run at 2 qblk and Lq = 1224 is what reaches two trips.  Padding rows hold random data.

Reference cost, measured on the CPU at these shapes (the restatement's per-key Python loops dominate; the oracle's quantisers are C): 0.02 -
0.17 s per sample of (b) and (c) -- 0.3 - 0.9 s per chunk of eight q_start samples, 0.3 - 0.65 s per chunk of six windows -- 0.17 s for the
packed bottom-right batch and 0.45 - 0.8 s per part of the packed window groups; (a) and (d) compare GPU results only.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loop_plan as lp
import ref_varlen_br as rb
import ref_varlen_window as rvw
import ref_window as rw
import util

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, core as sc, ops, quant as sq
    DEV = torch.device("cuda:0")

HQ, HKV, LQ, LKP = 2, 1, lp.LQ, lp.LKP
F16, BF16 = torch.float16, torch.bfloat16
DS = (128, 64)
FP8 = lambda *a, **kw: sa.sageattn_qk_int8_pv_fp8_cuda(*a, **kw)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _chunks(seq, n):
    return [tuple(seq[i:i + n]) for i in range(0, len(seq), n)]


def _ints(values, dtype=torch.int32):
    return torch.tensor(list(values), dtype=dtype, device=DEV)


def _same(a, b, what=""):
    assert torch.equal(a[0], b[0]), f"{what}: o differs in {int((a[0] != b[0]).sum())} of {a[0].numel()} elements"
    assert torch.equal(a[1], b[1]), f"{what}: lse differs in {int((a[1] != b[1]).sum())} of {a[1].numel()} rows"


@functools.lru_cache(maxsize=None)
def _qkv(D, dt, nb, hq=HQ, lq=LQ, seed=29):
    """q [nb, hq, lq, D], k / v [nb, HKV, LKP, D] (HND, K with a per-channel bias), on the device: made once per shape, never modified."""
    g = torch.Generator().manual_seed(seed + D + lq + 7 * hq)
    q = torch.randn(nb, hq, lq, D, generator=g).to(dt)
    k = (torch.randn(nb, HKV, LKP, D, generator=g) + torch.randn(1, HKV, 1, D, generator=g)).to(dt)
    v = torch.randn(nb, HKV, LKP, D, generator=g).to(dt)
    return q.to(DEV), k.to(DEV), v.to(DEV)


def _forms(plans):
    return " ".join(f"blk{j}{lp.describe(p)}" for j, p in enumerate(plans) if p.exists)


# ---------------------------------------------------------------------------------------------- the predicate restatement (b, c, the random sweep)
def ref_sample(oracle, qb, kb, vb, code, D, smooth_k, keep):
    """Reference o (float32 [Hq, lq, D]) and lse (natural log, as the entry point returns it) of one sample under the predicate ``keep`` [lq, n]
    -- test_gpu_window.py::_ref_sample for any number of heads.  qb / kb / vb: HND batches of one on the device, kb / vb cut to the n valid keys."""
    hq, lq, hkv, n = qb.shape[1], qb.shape[2], kb.shape[1], kb.shape[2]
    if n == 0:
        return np.zeros((hq, lq, D), np.float32), np.full((hq, lq), -np.inf, np.float32)
    km = None
    if smooth_k:
        km = util.bits(sq.channel_mean(kb if D in (64, 128) else F.pad(kb, (0, 128 - D))))
    _, _, aux = oracle.sageattn_dense(util.bits(qb), util.bits(kb), util.bits(vb), code, is_causal=True, pv="f8", qk_quant_gran="per_thread",
                                      return_lse=True, km=km, smooth_k=smooth_k, fp8_scores="exact")
    o, lse = rw.attn_window(aux["q8"][0], aux["k8"][0], aux["v8"][0], aux["qs"][0], aux["gq"], aux["ks"][0], aux["gk"], aux["vs"][0], keep,
                            c=np.float32(aux["c"]), out_dtype=F16 if code == 0 else BF16)
    lse = lse.numpy() / np.float32(oracle.LOG2E)
    if smooth_k:      # sageattn_dense's own LSE post-processing: + q . km * sm_scale, the product rounded to the input dtype
        kind = "f16" if code == 0 else "bf16"
        qf = oracle.to_f32(util.bits(qb if D in (64, 128) else F.pad(qb, (0, 128 - D))), code)
        kmf = np.repeat(oracle.to_f32(aux["km"], code), hq // hkv, axis=1)
        corr = oracle.to_f32(oracle.convert(np.einsum("bhld,bhd->bhl", qf, kmf), kind), code)
        lse = lse + corr[0] * np.float32(1.0 / (D ** 0.5))
    return o.float().numpy()[..., :D], lse


def check_sample(oracle, tag, qb, kb, vb, code, D, smooth_k, keep, ob, lb):
    """One sample against the restatement at test_gpu_window.py::_check's bar: ``2e-3 max|ref| + 2 output ulps``, LSE within 5e-3, rows without
    keys exactly +0 / -inf and the predicate's.  ob [1, Hq, lq, D] (HND), lb [1, Hq, lq] on the device."""
    hq, lq = qb.shape[1], qb.shape[2]
    ref, lse_ref = ref_sample(oracle, qb, kb, vb, code, D, smooth_k, keep)
    got, lgot = ob[0].float().cpu().numpy(), lb[0].cpu().numpy()
    empty = np.broadcast_to(~keep.any(dim=1).numpy(), (hq, lq))
    assert np.array_equal(np.isneginf(lse_ref), empty), tag
    scale = float(np.abs(ref).max())
    bar = 2e-3 * scale + 2 * util.out_ulp(scale, code)                  # (tests/test_gpu_window.py::_check)
    err = float(np.abs(got - ref).max())
    lerr = float(np.abs(lgot[~empty] - lse_ref[~empty]).max()) if (~empty).any() else 0.0
    print(f"{tag}: max|diff| {err:.3e} (bar {bar:.3e}), lse {lerr:.3e}, {int(empty[0].sum())} empty rows")
    assert np.isfinite(got).all() and not np.isnan(lgot).any(), tag
    assert np.array_equal(np.isneginf(lgot), empty), tag                 # the rows without keys are the predicate's
    assert not got[empty].any() and not np.signbit(got[empty]).any(), tag       # +0, not merely small
    assert err <= bar, (tag, err, bar)
    assert lerr <= 5e-3, (tag, lerr)                                     # (tests/test_gpu_window.py::_check)


def ref_sample_quantised(oracle, q_bits, k8, k_scale, v8, v_scale, k_mean, code, D, keep):
    """``ref_sample`` for keys and values that are QUANTISED ALREADY (tests/test_gpu_kvcache_programs.py: the operands a cache's ledger derives):
    q_bits uint16 ``[Hq, lq, D]`` is quantised by the oracle as the fused quantiser does (per-thread groups, 32-row warps of a 128-row block);
    k8 int8 / v8 e4m3 bytes ``[Hkv, n, D]``, k_scale fp32 ``[Hkv, 4 * ceil(n / 64)]``, v_scale fp32 ``[Hkv, D]``; k_mean: the uint16 bits
    ``[Hkv, D]`` the keys were smoothed with, or None -- the LSE takes ``q . k_mean * sm_scale`` as ``ref_sample`` forms it.  numpy only."""
    hq, lq = q_bits.shape[:2]
    hkv, n = k8.shape[:2]
    if n == 0 or lq == 0:
        return np.zeros((hq, lq, D), np.float32), np.full((hq, lq), -np.inf, np.float32)
    gq, nq = oracle.group_index(lq, "per_thread", "q", 128, 32)
    gk, nk = oracle.group_index(n, "per_thread", "k", 64, 64)
    assert k_scale.shape == (hkv, nk)
    q8, qs = oracle.quant_int8(np.ascontiguousarray(q_bits)[None], code, gq, nq, style=oracle.STYLE_TRITON_THREAD)
    sm_scale = 1.0 / (D ** 0.5)
    c = np.float32(sm_scale) * np.float32(oracle.LOG2E)                 # (oracle.sageattn_dense, per_thread)
    o, lse = rw.attn_window(q8[0], k8, v8, qs[0], gq, k_scale, gk, v_scale, keep, c=np.float32(c), out_dtype=F16 if code == 0 else BF16)
    lse = lse.numpy() / np.float32(oracle.LOG2E)
    if k_mean is not None:
        kind = "f16" if code == 0 else "bf16"
        kmf = np.repeat(oracle.to_f32(np.ascontiguousarray(k_mean), code), hq // hkv, axis=0)
        corr = oracle.to_f32(oracle.convert(np.einsum("hld,hd->hl", oracle.to_f32(np.ascontiguousarray(q_bits), code), kmf), kind), code)
        lse = lse + corr * np.float32(sm_scale)
    return o.float().numpy(), lse


def check_sample_quantised(oracle, tag, q_bits, k8, k_scale, v8, v_scale, k_mean, code, D, keep, got, lgot):
    """``check_sample`` on quantised keys and values, at its bar: ``2e-3 max|ref| + 2 output ulps``, LSE within 5e-3, rows without keys exactly
    +0 / -inf and the predicate's.  got float32 ``[Hq, lq, D]``, lgot float32 ``[Hq, lq]`` (numpy).  Returns (err / bar, the LSE error)."""
    hq, lq = q_bits.shape[:2]
    ref, lse_ref = ref_sample_quantised(oracle, q_bits, k8, k_scale, v8, v_scale, k_mean, code, D, keep)
    keep = keep if isinstance(keep, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(keep))
    empty = np.broadcast_to(~keep.any(dim=1).numpy() if keep.shape[1] else np.ones((lq,), bool), (hq, lq))
    assert np.array_equal(np.isneginf(lse_ref), empty), tag
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    bar = 2e-3 * scale + 2 * util.out_ulp(scale, code)                  # (check_sample)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    lerr = float(np.abs(lgot[~empty] - lse_ref[~empty]).max()) if (~empty).any() else 0.0
    print(f"{tag}: max|diff| {err:.3e} (bar {bar:.3e}), lse {lerr:.3e}, {int(empty[0].sum()) if hq else 0} empty rows")
    assert np.isfinite(got).all() and not np.isnan(lgot).any(), tag
    assert np.array_equal(np.isneginf(lgot), empty), tag                 # the rows without keys are the predicate's
    assert not got[empty].any() and not np.signbit(got[empty]).any(), tag       # +0, not merely small
    assert err <= bar, (tag, err, bar)
    assert lerr <= 5e-3, (tag, lerr)
    return (err / bar if bar > 0 else 0.0), lerr


# ---------------------------------------------------------------------------------------------- a. kv_lens
@pytest.mark.parametrize("causal", [False, True], ids=["nc", "causal"])
@pytest.mark.parametrize("D", DS)
def test_kv_lens_every_sample_is_the_plain_call_on_its_slice(D, causal):
    """One call on all lengths of the table; each sample equals the plain call on its slice, o and lse, bit for bit
    (test_gpu_kv_lens.py::test_every_sample_is_the_plain_call_on_its_slice).  The plain call runs the ``f8`` units, this one ``f8k``."""
    dt = (F16, BF16)[(DS.index(D) + causal) & 1]
    lens, lq = lp.KV_LENS, lp.LQ_CAUSAL_LENS if causal else LQ
    q, k, v = _qkv(D, dt, len(lens), lq=lq)
    # (smooth_k=False: with it the entry point adds q . km to the lse, a torch matmul whose last bit depends on the batch it is called with --
    #  test_gpu_q_start.py says the same of its padded call -- and nothing of the attention loop depends on it)
    kw = dict(is_causal=causal, smooth_k=False, return_lse=True)
    o, lse = FP8(q, k, v, kv_lens=_ints(lens), **kw)
    assert o.shape == q.shape and lse.shape == (len(lens), HQ, lq)
    plans = lp.kv_lens_plans(causal)
    bad = []
    for b, n in enumerate(lens):
        forms = sorted({lp.describe(plans[n, j]) for j in range(lp.nblk(lq))})
        if n == 0:
            same = bool((o[b] == 0).all()) and bool(torch.isneginf(lse[b]).all())
        else:
            ob, lb = FP8(q[b:b + 1], k[b:b + 1, :, :n].contiguous(), v[b:b + 1, :, :n].contiguous(), **kw)
            same = torch.equal(o[b:b + 1], ob) and torch.equal(lse[b:b + 1], lb)
            if not same:
                bad.append((n, int((o[b:b + 1] != ob).sum()), int((lse[b:b + 1] != lb).sum())))
        print(f"len {n}: {'same bits' if same else 'DIFFERS'}; {' '.join(forms)}")
    assert not bad, f"(len, differing o elements, differing lse rows): {bad}"
    assert bool(torch.isfinite(o.float()).all()) and not bool(torch.isnan(lse).any())


# ---------------------------------------------------------------------------------------------- b. q_start
@pytest.mark.parametrize("D", DS)
def test_q_start_multiples_of_128_are_the_padded_plain_call(D):
    """test_gpu_q_start.py::test_aligned_offsets_are_the_padded_plain_call at offsets up to 1024: the same query blocks and Q groups, every work item
    the same tiles through the same bodies, in the ``f8q`` unit here and the ``f8`` unit there."""
    dt = (F16, BF16)[DS.index(D)]
    pairs = lp.Q_START_ALIGNED
    q, k, v = _qkv(D, dt, len(pairs))
    junk = (3.0 * torch.randn(1, HQ, max(s for _, s in pairs), D, generator=torch.Generator().manual_seed(5))).to(dt).to(DEV)
    kw = dict(is_causal=True, smooth_k=False, return_lse=True)
    o, lse = FP8(q, k, v, kv_lens=_ints([n for n, _ in pairs]), q_start=_ints([s for _, s in pairs]), **kw)
    plans = lp.q_start_plans(pairs)
    for b, (n, s) in enumerate(pairs):
        op, lp_ = FP8(torch.cat((junk[:, :, :s], q[b:b + 1]), dim=2), k[b:b + 1, :, :n].contiguous(), v[b:b + 1, :, :n].contiguous(), **kw)
        print(f"len {n} offset {s}: {_forms([plans[n, s, j] for j in range(2)])}")
        _same((o[b:b + 1], lse[b:b + 1]), (op[:, :, s:], lp_[:, :, s:]), f"len {n}, offset {s}")
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all())


Q_START_CHUNKS = _chunks(lp.Q_START_PAIRS, 8)


@pytest.mark.parametrize("chunk", range(len(Q_START_CHUNKS)))
@pytest.mark.parametrize("D", DS)
def test_q_start_any_offset_vs_restatement(oracle_mod, D, chunk):
    pairs = Q_START_CHUNKS[chunk]
    dt, smooth_k = (F16, BF16)[(chunk + DS.index(D)) & 1], bool(chunk & 1)
    code = 0 if dt == F16 else 1
    q, k, v = (t[:len(pairs)] for t in _qkv(D, dt, 8))
    o, lse = FP8(q, k, v, kv_lens=_ints([n for n, _ in pairs]), q_start=_ints([s for _, s in pairs]), is_causal=True, smooth_k=smooth_k, return_lse=True)
    plans = lp.q_start_plans(pairs)
    for b, (n, s) in enumerate(pairs):
        keep = rw.visible(LQ, n, s, 0, 0, n)
        tag = f"d{D} len {n} offset {s} {_forms([plans[n, s, j] for j in range(2)])}"
        check_sample(oracle_mod, tag, q[b:b + 1], k[b:b + 1, :, :n].contiguous(), v[b:b + 1, :, :n].contiguous(), code, D, smooth_k, keep,
                     o[b:b + 1], lse[b:b + 1])


# ---------------------------------------------------------------------------------------------- c. window_size
WINDOW_CHUNKS = _chunks(lp.window_cases(), 6)


@pytest.mark.parametrize("chunk", range(len(WINDOW_CHUNKS)))
@pytest.mark.parametrize("D", DS)
def test_windows_vs_restatement(oracle_mod, D, chunk):
    """The window is one per call: every case is its own call on the chunk's batch (its length and offset in its slot), and its slot is checked
    (test_gpu_window.py::test_windows_vs_restatement)."""
    cases = WINDOW_CHUNKS[chunk]
    plans = lp.window_plans()
    lens, starts = [c[0] for c in cases], [c[1] for c in cases]
    for b, (n, s, W) in enumerate(cases):
        dt, smooth_k = (F16, BF16)[(6 * chunk + b + DS.index(D)) & 1], bool((chunk + b) & 2)
        code = 0 if dt == F16 else 1
        q, k, v = (t[:len(cases)] for t in _qkv(D, dt, 6))
        o, lse = FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints(starts), window_size=(W - 1, 0), is_causal=True, smooth_k=smooth_k, return_lse=True)
        keep = rw.visible(LQ, n, s, W, 0, n)
        tag = f"d{D} len {n} offset {s} window {W} {_forms([plans[n, s, W, j] for j in range(2)])}"
        check_sample(oracle_mod, tag, q[b:b + 1], k[b:b + 1, :, :n].contiguous(), v[b:b + 1, :, :n].contiguous(), code, D, smooth_k, keep,
                     o[b:b + 1], lse[b:b + 1])


# ---------------------------------------------------------------------------------------------- d. pack_gqa
PACK_CASES = [(route, lq, group, DS[(r + i) & 1]) for r, route in enumerate(("lens", "qstart", "window"))
              for i, (lq, group) in enumerate((lq, g) for lq in lp.PACK_LQS for g in lp.PACK_GROUPS)]
assert {(c[0], c[1], c[2]) for c in PACK_CASES} == {(r, lq, g) for r in ("lens", "qstart", "window") for lq in lp.PACK_LQS for g in lp.PACK_GROUPS}
assert {(c[0], c[3]) for c in PACK_CASES} == {(r, D) for r in ("lens", "qstart", "window") for D in DS}


@pytest.mark.parametrize("case", PACK_CASES, ids=[f"{r}-lq{lq}-g{g}-d{D}" for r, lq, g, D in PACK_CASES])
def test_pack_gqa_equals_the_unpacked_call_bit_for_bit(case):
    """The tables of (a) - (c) at decode shapes: groups of 4 (every wave busy) and 5 (a second block with three idle waves)."""
    route, lq, group, D = case
    dt = (F16, BF16)[(lq + group) & 1]
    plans = lp.pack_plans(route, lq)
    if route == "lens":
        calls = [(dict(is_causal=False, kv_lens=list(lp.KV_LENS)), [(n,) for n in lp.KV_LENS])]
    elif route == "qstart":
        pairs = lp.Q_START_ALIGNED + lp.Q_START_PAIRS
        calls = [(dict(is_causal=True, kv_lens=[n for n, _ in pairs], q_start=[s for _, s in pairs]), list(pairs))]
    else:
        calls = [(dict(is_causal=True, kv_lens=[c[0] for c in chunk], q_start=[c[1] for c in chunk], window_size=(W - 1, 0)), [(n, s, W)])
                 for chunk in WINDOW_CHUNKS for n, s, W in chunk]
    probe = ctypes.c_int32(-1)
    for kw, keys in calls:
        nb = len(kw["kv_lens"])
        q, k, v = (t[:nb] for t in _qkv(D, dt, 64, hq=group * HKV, lq=lq))
        kw = {a: (_ints(b) if isinstance(b, list) else b) for a, b in kw.items()}
        probe.value = -1
        with ops.launch_hooks(grid_probe=probe):
            got = FP8(q, k, v, return_lse=True, pack_gqa=True, **kw)
        torch.cuda.synchronize()
        assert probe.value == nb * HKV * ((group + 3) // 4), (probe.value, nb, group)          # (test_gpu_gqa_pack.py::test_the_packed_route_ran)
        with ops.launch_hooks(grid_probe=probe):
            want = FP8(q, k, v, return_lse=True, pack_gqa=False, **kw)
        torch.cuda.synchronize()
        assert probe.value == nb * group * HKV, (probe.value, nb, group)
        print(f"{route} lq {lq} group {group}: " + " ".join(f"{key}{lp.describe(plans[key])}" for key in keys))
        _same(got, want, f"{route}, {keys if len(keys) == 1 else len(keys)} samples")
        assert not bool(torch.isnan(got[0].float()).any()) and not bool(torch.isnan(got[1]).any())


# ---------------------------------------------------------------------------------------------- e. the packed launches
BR = dict(is_causal=True, causal_align="bottom_right")


def _tdt(dt):
    return F16 if dt == 0 else BF16


@functools.lru_cache(maxsize=None)
def _packed_inputs(pairs, hq, hkv, D, dt, seed):
    """test_gpu_varlen_br.py::_inputs: q [sum Lq, hq, D], k / v [sum Lk, hkv, D] on the CPU, cu_q, cu_k."""
    lq, lk = [p[0] for p in pairs], [p[1] for p in pairs]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(sum(lq), hq, D, generator=g).to(_tdt(dt))
    k = (torch.randn(sum(lk), hkv, D, generator=g) + torch.randn(1, hkv, D, generator=g)).to(_tdt(dt))
    v = torch.randn(sum(lk), hkv, D, generator=g).to(_tdt(dt))
    cu = lambda lens: torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    return q, k, v, cu(lq), cu(lk)


def _packed_run(ins, **kw):
    q, k, v, cu_q, cu_k = ins
    mq, mk = max(int((cu_q[1:] - cu_q[:-1]).max()), 1), max(int((cu_k[1:] - cu_k[:-1]).max()), 1)
    out = sa.sageattn_qk_int8_pv_fp8_varlen(q.to(DEV), k.to(DEV), v.to(DEV), cu_q.to(DEV), cu_k.to(DEV), mq, mk, **kw)
    torch.cuda.synchronize()
    return out


def _km_of_call(k, cu_q, cu_k):
    """The K mean the call forms (test_gpu_varlen_br.py::_km_of_call): over all packed tokens, summed over the plan's per-sequence slabs."""
    kd, cq, ck = sc._pad_head_dim(*(k.to(DEV),) * 3)[0], cu_q.to(DEV), cu_k.to(DEV)
    return util.bits(sq.channel_mean_packed(kd, ck, sq.varlen_plan(cq, ck, total_q=int(cu_q[-1]), total_k=k.shape[0])))


def _check_packed(O, ins, dt, W, o, lse, tag, plans):
    """Every sequence against the restatement: W = 0 ``ref_varlen_br`` at test_gpu_varlen_br.py::_check_vs_oracle's bar (2e-3 max|o| + one
    output ulp), W > 0 ``ref_varlen_window`` at test_gpu_varlen_window.py::_check_vs_reference's (two ulps); LSE within 5e-3; rows without
    keys exactly +0 / -inf by closed form."""
    q, k, v, cu_q, cu_k = ins
    km = _km_of_call(k, cu_q, cu_k)
    if W:
        ref_bits, lse_ref = rvw.ref_f8_varlen_window(O, util.bits(q), util.bits(k), util.bits(v), dt, cu_q.numpy(), cu_k.numpy(), W, km=km, return_lse=True)
    else:
        ref_bits, lse_ref = rb.oracle_f8_varlen_br(O, util.bits(q), util.bits(k), util.bits(v), dt, cu_q.numpy(), cu_k.numpy(), km=km, return_lse=True)
    ref, got, lgot = util.f32(ref_bits, dt), o.float().cpu().numpy(), lse.cpu().numpy()
    assert np.isfinite(got).all() and not np.isnan(lgot).any(), tag
    empty = np.isneginf(lse_ref)
    assert np.array_equal(np.isneginf(lgot), empty), tag
    for b in range(len(cu_q) - 1):
        s, e = int(cu_q[b]), int(cu_q[b + 1])
        lq, lk = e - s, int(cu_k[b + 1] - cu_k[b])
        if lq == 0:
            continue
        none = rb.rows_without_keys(lq, lk)
        assert empty[:, s:e].sum() == q.shape[1] * none and empty[:, s:s + none].all(), (tag, b)
        assert not got[s:s + none].any() and not np.signbit(got[s:s + none]).any(), (tag, b)
        scale = float(np.abs(ref[s:e]).max())
        bar = 2e-3 * scale + (2 if W else 1) * util.out_ulp(scale, dt)
        err = float(np.abs(got[s:e] - ref[s:e]).max())
        seen = ~empty[:, s:e]
        lerr = float(np.abs(lgot[:, s:e][seen] - lse_ref[:, s:e][seen]).max()) if seen.any() else 0.0
        print(f"{tag} seq {b} (Lq {lq}, Lk {lk}) {_forms([plans[lq, lk, j] for j in range(lp.nblk(lq))])}: max|diff| {err:.3e} (bar {bar:.3e}), "
              f"lse {lerr:.3e}, {none} rows without keys")
        assert err <= bar, (tag, b, err, bar)
        assert lerr <= 5e-3, (tag, b, lerr)


@pytest.mark.parametrize("D", DS)
def test_packed_bottom_right_vs_oracle(oracle_mod, D):
    dt = DS.index(D)
    pairs = lp.packed_br_pairs()
    ins = _packed_inputs(pairs, HQ, HKV, D, dt, 301 + D)
    o, lse = _packed_run(ins, return_lse=True, **BR)
    _check_packed(oracle_mod, ins, dt, 0, o, lse, f"br/d{D}", lp.packed_plans(0, pairs))


WINDOW_GROUPS = lp.packed_window_cases()
WINDOW_PARTS = _chunks(WINDOW_GROUPS, 5)


@pytest.mark.parametrize("part", range(len(WINDOW_PARTS)))
@pytest.mark.parametrize("D", DS)
def test_packed_windows_vs_reference(oracle_mod, D, part):
    """The window is one per call: one packed call per window of the selection."""
    for i, (W, pairs) in enumerate(WINDOW_PARTS[part]):
        dt = (i + part + DS.index(D)) & 1
        ins = _packed_inputs(pairs, HQ, HKV, D, dt, 401 + D + W)
        o, lse = _packed_run(ins, return_lse=True, window_size=(W - 1, 0), **BR)
        _check_packed(oracle_mod, ins, dt, W, o, lse, f"window {W}/d{D}", lp.packed_plans(W, pairs))


def _ticket_batch(pairs, D):
    """The sequences repeated until a launch of 32 query heads has two rounds of workgroups, from where the ticket route can be forced
    (512 resident workgroups at D = 128, 768 at D = 64)."""
    blocks = sum(lp.nblk(lq) for lq, _ in pairs)
    reps = -(-2 * (512 if D == 128 else 768) // (32 * blocks))
    return tuple(pairs) * reps


@pytest.mark.parametrize("D", DS)
def test_packed_ticket_route_equals_the_ordinary_launch(monkeypatch, D):
    """Each batch of (e) once more on the ticket route (persistent workgroups over the work list), bit-identical to its ordinary launch; the
    probe confirms the route (test_gpu_varlen_window.py::test_ticket_route_equals_the_ordinary_launch)."""
    probe = ctypes.c_int32(-1)
    for W, pairs in ((0, lp.packed_br_pairs()),) + WINDOW_GROUPS:
        batch = _ticket_batch(pairs, D)
        ins = _packed_inputs(batch, 32, 4, D, 1, 501 + D + W)
        kw = dict(BR, window_size=(W - 1, 0)) if W else BR
        monkeypatch.setattr(ops, "_PERSISTENT", False)
        with ops.launch_hooks(grid_probe=probe):
            want = _packed_run(ins, return_lse=True, **kw)
        ordinary = probe.value
        monkeypatch.setattr(ops, "_PERSISTENT", True)
        with ops.launch_hooks(grid_probe=probe, force_persistent=True):
            got = _packed_run(ins, return_lse=True, **kw)
        assert 0 < probe.value < ordinary, (W, probe.value, ordinary)
        _same(got, want, f"tickets, window {W}")
        assert not bool(torch.isnan(got[0].float()).any())
