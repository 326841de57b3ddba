"""GPU: sageattn_qk_int8_pv_fp8_varlen -- FP8 (e4m3) PV for packed variable-length batches.

  * against an oracle composed here from oracle/__init__.py's building blocks: sageattn_varlen's Q / K half (per-block INT8, Triton
    rounding, sm_scale log2(e) in Q, K smoothed by the mean over ALL packed tokens), V in e4m3 with one scale per (sequence, kv-head,
    channel), the exact FP8 score form, two-level or single accumulation; every sequence held to 2e-3 max|o| + one output ulp, the LSE
    to the dense FP8 return_lse bar (5e-3);
  * bit identities: the Q / K bits of sageattn_varlen, the V pre-pass bits of per_channel_fp8 on each sequence alone, the route
    switches, and the isolation of a sequence from the others of its batch (per-sequence V scales).
"""
import numpy as np
import pytest
import torch

import util

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, core as sc, quant as sq
    DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _tdt(dt):
    return torch.float16 if dt == 0 else torch.bfloat16


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)


def _qkv(lens_q, lens_k, Hq, Hkv, D, dt, seed, k_shift=1.5):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(int(sum(lens_q)), Hq, D, generator=g).to(_tdt(dt))
    k = (torch.randn(int(sum(lens_k)), Hkv, D, generator=g) + k_shift).to(_tdt(dt))
    v = torch.randn(int(sum(lens_k)), Hkv, D, generator=g).to(_tdt(dt))
    return q, k, v


def _km_of_call(k, cu_q, cu_k, use_plan=True):
    """The K mean the call forms: over ALL packed tokens, summed over the plan's per-sequence slabs (or packed slabs without a plan)."""
    kd, cq, ck = sc._pad_head_dim(*(k.to(DEV),) * 3)[0], cu_q.to(DEV), cu_k.to(DEV)
    plan = sq.varlen_plan(cq, ck, total_q=int(cu_q[-1]), total_k=k.shape[0]) if use_plan else None
    return util.bits(sq.channel_mean_packed(kd, ck, plan))


def oracle_f8_varlen(O, q, k, v, dt, cu_q, cu_k, *, causal, km, single=False, sm_scale=None, return_lse=False):
    """The new route on packed [sum L, H, D] bit arrays: oracle.sageattn_varlen's Q / K half, per-sequence quant_v_fp8, attn(FP8 PV, c = 1,
    exact scores).  km: bits [1, Hkv, D] or None (smooth_k=False).  Returns (o bits [sum Lq, Hq, D0], lse [Hq, sum Lq] natural log | None)."""
    D0 = q.shape[-1]
    q, k, v = (O._pad_head_dim(t, dt) for t in (q, k, v))
    Hq, Hkv, D = q.shape[1], k.shape[1], q.shape[2]
    if sm_scale is None:
        sm_scale = 1.0 / (D0 ** 0.5)
    kind = "f16" if dt == 0 else "bf16"
    if km is not None:
        kmp = np.zeros((1, Hkv, D), dtype=np.uint16)
        kmp[..., :D0] = np.asarray(km).reshape(1, Hkv, -1)[..., :D0]
        kmf = O.to_f32(kmp, dt)
        k = O.convert(O.to_f32(k, dt) - kmf, kind)
    o = np.zeros(q.shape, dtype=np.uint16)
    lse = np.full((Hq, q.shape[0]), -np.inf, dtype=np.float32) if return_lse else None
    for b in range(len(cu_q) - 1):
        qs_, qe = int(cu_q[b]), int(cu_q[b + 1])
        ks_, ke = int(cu_k[b]), int(cu_k[b + 1])
        if qe == qs_ or ke == ks_:          # no rows, or no keys: zero output, lse -inf
            continue
        qb = np.ascontiguousarray(q[qs_:qe].transpose(1, 0, 2))[None]
        kb = np.ascontiguousarray(k[ks_:ke].transpose(1, 0, 2))[None]
        vb = np.ascontiguousarray(v[ks_:ke].transpose(1, 0, 2))[None]
        gq, nq = O.group_index(qe - qs_, "per_block", "q", 128, 128)
        gk, nk = O.group_index(ke - ks_, "per_block", "k", 64, 64)
        q8, qsc = O.quant_int8(qb, dt, gq, nq, pre_scale=np.float32(sm_scale * O.LOG2E), style=O.STYLE_TRITON)
        k8, ksc = O.quant_int8(kb, dt, gk, nk, style=O.STYLE_TRITON)
        v8, vs = O.quant_v_fp8(vb, dt)
        ob, lb = O.attn(q8, k8, v8, qsc, gq, ksc, gk, causal=causal, c=1.0, pv_mode=O.PV_F8_SINGLE if single else O.PV_F8_TWO_LEVEL,
                        out_dtype=dt, v_scale=vs, return_lse=return_lse, score_mode=O.SCORES_EXACT)
        o[qs_:qe] = ob[0].transpose(1, 0, 2)
        if return_lse:
            lse[:, qs_:qe] = lb[0]
    if return_lse:
        lse = lse / np.float32(O.LOG2E)
        if km is not None:            # q . km per (head, row) in the input dtype, * sm_scale (core.py:289-293,328-329)
            kmq = np.repeat(O.to_f32(np.asarray(km).reshape(1, Hkv, -1), dt)[0, :, :D0], Hq // Hkv, axis=0)     # [Hq, D0]
            corr = np.einsum("thd,hd->ht", O.to_f32(q[..., :D0], dt), kmq)
            lse = lse + O.to_f32(O.convert(corr.astype(np.float32), kind), dt) * np.float32(sm_scale)
    return np.ascontiguousarray(o[..., :D0]), lse


def _assert_per_sequence(tag, got, ref_bits, dt, cu_q):
    """Every sequence: max|diff| <= 2e-3 max|o| + one output ulp at max|o| (the bar of the default dense routes)."""
    ref = util.f32(ref_bits, dt)
    assert np.isfinite(got).all(), tag
    for b in range(len(cu_q) - 1):
        s, e = int(cu_q[b]), int(cu_q[b + 1])
        if e == s:
            continue
        scale = float(np.abs(ref[s:e]).max())
        err = float(np.abs(got[s:e] - ref[s:e]).max())
        assert err <= 2e-3 * scale + util.out_ulp(scale, dt), f"{tag} seq {b} (rows {s}:{e}): max|diff| {err:.3e} vs max|o| {scale:.3e}"


def _run(q, k, v, cu_q, cu_k, causal, **kw):
    lq = (cu_q[1:] - cu_q[:-1]).max().item()
    lk = (cu_k[1:] - cu_k[:-1]).max().item()
    out = sa.sageattn_qk_int8_pv_fp8_varlen(q.to(DEV), k.to(DEV), v.to(DEV), cu_q.to(DEV), cu_k.to(DEV), max(int(lq), 1), max(int(lk), 1),
                                            is_causal=causal, **kw)
    torch.cuda.synchronize()
    return out


LENS = [1, 63, 64, 0, 65, 127, 129, 1000]


@pytest.mark.parametrize("accum", ["fp32+fp32", "fp32"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128, 40, 96])
@pytest.mark.parametrize("dt", [0, 1])
def test_matches_oracle(oracle_mod, dt, D, causal, accum):
    """GQA 4/1, the ragged lengths around the 64-key tiles and 128-row blocks, an empty sequence; head dims padded as sageattn_varlen pads."""
    cu = _cu(LENS)
    q, k, v = _qkv(LENS, LENS, 4, 1, D, dt, seed=D + 7 * dt + 3 * causal)
    o = _run(q, k, v, cu, cu, causal, pv_accum_dtype=accum)
    assert o.shape == q.shape and o.dtype == q.dtype
    ref, _ = oracle_f8_varlen(oracle_mod, util.bits(q), util.bits(k), util.bits(v), dt, cu.numpy(), cu.numpy(), causal=causal,
                              km=_km_of_call(k, cu, cu), single=accum == "fp32")
    _assert_per_sequence(f"d{D}/dt{dt}/{'c' if causal else 'nc'}/{accum}", o.float().cpu().numpy(), ref, dt, cu.numpy())


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dt", [0, 1])
def test_gqa_32_8(oracle_mod, dt, causal):
    lens = [129, 300, 65, 1, 256]
    cu = _cu(lens)
    q, k, v = _qkv(lens, lens, 32, 8, 128, dt, seed=11 + dt + 2 * causal)
    o = _run(q, k, v, cu, cu, causal)
    ref, _ = oracle_f8_varlen(oracle_mod, util.bits(q), util.bits(k), util.bits(v), dt, cu.numpy(), cu.numpy(), causal=causal,
                              km=_km_of_call(k, cu, cu))
    _assert_per_sequence(f"gqa32_8/dt{dt}/{'c' if causal else 'nc'}", o.float().cpu().numpy(), ref, dt, cu.numpy())


@pytest.mark.parametrize("accum", ["fp32+fp32", "fp32"])
@pytest.mark.parametrize("causal", [False, True])
def test_one_sequence_longer_than_4096(oracle_mod, causal, accum):
    """H 1/1: a sequence of 4161 tokens (the pipelined loops' steady state, the last-tile bodies) between short ones; the last sequence
    of the batch ends in a ragged tile (no K / V read past the packed buffer)."""
    lens = [70, 4161, 1, 190]
    cu = _cu(lens)
    q, k, v = _qkv(lens, lens, 1, 1, 128, 1, seed=5 + causal)
    o = _run(q, k, v, cu, cu, causal, pv_accum_dtype=accum)
    ref, _ = oracle_f8_varlen(oracle_mod, util.bits(q), util.bits(k), util.bits(v), 1, cu.numpy(), cu.numpy(), causal=causal,
                              km=_km_of_call(k, cu, cu), single=accum == "fp32")
    _assert_per_sequence(f"long/{'c' if causal else 'nc'}/{accum}", o.float().cpu().numpy(), ref, 1, cu.numpy())


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dt,D", [(0, 64), (1, 128)])
def test_cu_q_differs_from_cu_k(oracle_mod, dt, D, causal):
    """Cross lengths (causal: top-left aligned within each sequence), an empty query side and an empty key side."""
    lq, lk = [100, 1, 0, 300, 64, 5], [257, 64, 30, 129, 200, 0]
    cu_q, cu_k = _cu(lq), _cu(lk)
    q, k, v = _qkv(lq, lk, 4, 2, D, dt, seed=31 + causal)
    o = _run(q, k, v, cu_q, cu_k, causal)
    ref, _ = oracle_f8_varlen(oracle_mod, util.bits(q), util.bits(k), util.bits(v), dt, cu_q.numpy(), cu_k.numpy(), causal=causal,
                              km=_km_of_call(k, cu_q, cu_k))
    _assert_per_sequence(f"cross/d{D}/{'c' if causal else 'nc'}", o.float().cpu().numpy(), ref, dt, cu_q.numpy())


@pytest.mark.parametrize("kind", ["x1000", "one_hot"])
def test_magnitudes_and_one_hot_rows(oracle_mod, kind):
    lens = [200, 65, 513]
    cu = _cu(lens)
    q, k, v = _qkv(lens, lens, 4, 2, 128, 0, seed=41)
    if kind == "x1000":
        q, k, v = ((t.float() * 1000.0).half() for t in (q, k, v))
    else:      # every query row one-hot in its own channel, keys one-hot: peaked softmax rows
        n = q.shape[0]
        q = torch.zeros_like(q)
        q[torch.arange(n), :, torch.arange(n) % 128] = 400.0
        k = torch.zeros_like(k)
        k[torch.arange(n), :, torch.arange(n) % 128] = 1.0
    for causal in (False, True):
        o = _run(q, k, v, cu, cu, causal)
        ref, _ = oracle_f8_varlen(oracle_mod, util.bits(q), util.bits(k), util.bits(v), 0, cu.numpy(), cu.numpy(), causal=causal,
                                  km=_km_of_call(k, cu, cu))
        _assert_per_sequence(f"{kind}/{'c' if causal else 'nc'}", o.float().cpu().numpy(), ref, 0, cu.numpy())


def test_more_sequences_than_the_plan_takes(oracle_mod):
    """1100 short sequences (> sage_varlen_plan_max_seqs()): no plan, the unit order, the statistics over slabs per sequence."""
    assert 1100 > _cabi.load().sage_varlen_plan_max_seqs()
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 40, size=1100)
    lens[7] = 130
    cu = _cu(lens)
    q, k, v = _qkv(lens, lens, 2, 1, 64, 1, seed=51)
    for causal in (False, True):
        o = _run(q, k, v, cu, cu, causal)
        ref, _ = oracle_f8_varlen(oracle_mod, util.bits(q), util.bits(k), util.bits(v), 1, cu.numpy(), cu.numpy(), causal=causal,
                                  km=_km_of_call(k, cu, cu, use_plan=False))
        _assert_per_sequence(f"many/{'c' if causal else 'nc'}", o.float().cpu().numpy(), ref, 1, cu.numpy())


@pytest.mark.parametrize("smooth_k", [True, False])
@pytest.mark.parametrize("accum", ["fp32+fp32", "fp32"])
@pytest.mark.parametrize("causal", [False, True])
def test_return_lse(oracle_mod, causal, accum, smooth_k):
    lq, lk = [129, 0, 64, 300], [129, 20, 64, 300] if causal else [200, 20, 1, 257]
    cu_q, cu_k = _cu(lq), _cu(lk)
    q, k, v = _qkv(lq, lk, 4, 2, 96, 0, seed=61 + causal)
    o, lse = _run(q, k, v, cu_q, cu_k, causal, pv_accum_dtype=accum, smooth_k=smooth_k, return_lse=True)
    o_plain = _run(q, k, v, cu_q, cu_k, causal, pv_accum_dtype=accum, smooth_k=smooth_k)
    assert torch.equal(o, o_plain)
    assert lse.dtype == torch.float32 and lse.shape == (4, q.shape[0])
    km = _km_of_call(k, cu_q, cu_k) if smooth_k else None
    ref, lse_ref = oracle_f8_varlen(oracle_mod, util.bits(q), util.bits(k), util.bits(v), 0, cu_q.numpy(), cu_k.numpy(), causal=causal,
                                    km=km, single=accum == "fp32", return_lse=True)
    _assert_per_sequence("lse/o", o.float().cpu().numpy(), ref, 0, cu_q.numpy())
    got = lse.cpu().numpy()
    empty = np.isneginf(lse_ref)                    # (rows of a sequence without keys)
    assert (np.isneginf(got) == empty).all()
    assert np.abs(got[~empty] - lse_ref[~empty]).max() <= 5e-3


def _prepare(q, k, v, cu_q, cu_k, v_fp8, **kw):
    lq = int((cu_q[1:] - cu_q[:-1]).max())
    lk = int((cu_k[1:] - cu_k[:-1]).max())
    st = sc._varlen_prepare(q.to(DEV), k.to(DEV), v.to(DEV), cu_q.to(DEV), cu_k.to(DEV), lq, lk, False, None, True, kw, v_fp8=v_fp8)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("fused_prepass", [True, False])
def test_q_and_k_bits_equal_sageattn_varlen(fused_prepass):
    lens = [300, 1, 64, 1000, 129]
    cu = _cu(lens)
    q, k, v = _qkv(lens, lens, 8, 2, 128, 1, seed=71)
    kw = dict(fuse_q_quant=False, fused_prepass=fused_prepass)
    a, b = _prepare(q, k, v, cu, cu, False, **kw), _prepare(q, k, v, cu, cu, True, **kw)
    nks, nqs = int(a.cu_ks[-1]), int(a.cu_qs[-1])
    assert torch.equal(a.k_int8, b.k_int8) and torch.equal(a.k_scale[:nks], b.k_scale[:nks])
    assert torch.equal(a.q_int8, b.q_int8) and torch.equal(a.q_scale[:nqs], b.q_scale[:nqs])
    assert torch.equal(a.cu_ks, b.cu_ks) and torch.equal(a.km, b.km)


@pytest.mark.parametrize("use_plan", [True, False])
@pytest.mark.parametrize("dt", [0, 1])
def test_v_prepass_equals_per_channel_fp8_of_each_sequence(oracle_mod, dt, use_plan):
    """The e4m3 image and scales of every sequence: the bits of the dense per_channel_fp8 (and of the oracle) on that sequence alone; the
    tail of a sequence's last tile zero; an empty sequence's scales zero."""
    lens = [65, 0, 1, 700, 128, 1100]
    cu = _cu(lens)
    _, _, v = _qkv(lens, lens, 1, 3, 128, dt, seed=81)
    v[700:701] *= 50                                   # an outlier token in sequence 3
    vd, cud = v.to(DEV), cu.to(DEV)
    plan = sq.varlen_plan(cud, cud, total_q=v.shape[0], total_k=v.shape[0]) if use_plan else None
    cu_ks = plan.cu_ks if plan is not None else sq._cu_blocks(cud, 64)
    img, vs = sq.per_channel_fp8_varlen(vd, cud, cu_ks, max(lens), plan=plan)
    torch.cuda.synchronize()
    img, vs, cu_ks = img.cpu().numpy(), vs.cpu().numpy(), cu_ks.cpu().numpy()
    for b, L in enumerate(lens):
        s = int(cu[b])
        if L == 0:
            assert (vs[b] == 0).all()
            continue
        vb = v[s:s + L].transpose(0, 1).unsqueeze(0).contiguous()              # [1, H, L, D]
        r8, rvs = oracle_mod.quant_v_fp8(util.bits(vb), dt)
        _, dvs, _ = sq.per_channel_fp8(vb.to(DEV))
        assert (vs[b] == rvs[0]).all() and (vs[b] == dvs[0].cpu().numpy()).all()
        tiles = img[cu_ks[b]:cu_ks[b + 1]]                                       # [nt, H, D, 64]
        assert tiles.shape[0] == (L + 63) // 64
        for h in range(3):
            full = util.decode_v_image(tiles[:, h], tiles.shape[0] * 64, fp8=True)
            assert (full[:L] == r8[0, h]).all() and (full[L:] == 0).all()


def test_route_switches_give_the_same_bits():
    lens = [300, 1, 0, 64, 1000, 129, 2100]
    cu = _cu(lens)
    q, k, v = _qkv(lens, lens, 8, 2, 128, 0, seed=91)
    for causal in (False, True):
        for accum in ("fp32+fp32", "fp32"):
            base, lse0 = _run(q, k, v, cu, cu, causal, pv_accum_dtype=accum, return_lse=True)
            for kw in (dict(fuse_q_quant=False), dict(work_list=False), dict(fused_prepass=False), dict(fused_prepass=True),
                       dict(fuse_q_quant=False, work_list=False)):
                o, lse = _run(q, k, v, cu, cu, causal, pv_accum_dtype=accum, return_lse=True, **kw)
                assert torch.equal(o, base), (causal, accum, kw)
                assert torch.equal(lse, lse0), (causal, accum, kw)
            # without the plan the K mean is summed over other slabs (equal up to an input-dtype rounding): same bits with smooth_k=False
            a = _run(q, k, v, cu, cu, causal, pv_accum_dtype=accum, smooth_k=False)
            for kw in (dict(varlen_plan=False), dict(varlen_plan=False, fuse_q_quant=False)):
                assert torch.equal(_run(q, k, v, cu, cu, causal, pv_accum_dtype=accum, smooth_k=False, **kw), a), (causal, accum, kw)


@pytest.mark.parametrize("causal", [False, True])
def test_sequence_isolation(causal):
    """smooth_k=False: sequence A's rows are bit-identical alone, as [A, B] with a V outlier x 1000 in B, and as [C, A]."""
    la, lb, lc = 333, 200, 90
    qa, ka, va = _qkv([la], [la], 4, 2, 128, 1, seed=101)
    qb, kb, vb = _qkv([lb], [lb], 4, 2, 128, 1, seed=102)
    qc, kc, vc = _qkv([lc], [lc], 4, 2, 128, 1, seed=103)
    vb[17] *= 1000
    alone = _run(qa, ka, va, _cu([la]), _cu([la]), causal, smooth_k=False)
    ab = _run(torch.cat([qa, qb]), torch.cat([ka, kb]), torch.cat([va, vb]), _cu([la, lb]), _cu([la, lb]), causal, smooth_k=False)
    ca = _run(torch.cat([qc, qa]), torch.cat([kc, ka]), torch.cat([vc, va]), _cu([lc, la]), _cu([lc, la]), causal, smooth_k=False)
    assert torch.equal(ab[:la], alone)
    assert torch.equal(ca[lc:], alone)


@pytest.mark.parametrize("causal", [False, True])
def test_ticket_route_equals_the_ordinary_launch(monkeypatch, causal):
    """Over the work list a large call runs as a persistent launch (causal: the CPERS instantiations): forced from two rounds of workgroups
    up, its bits equal the ordinary launch's, and the probe confirms that the route was taken."""
    import ctypes
    from sageattention_amd import ops
    lens = [256, 7000, 1, 3000, 6100, 511]
    cu = _cu(lens)
    q, k, v = _qkv(lens, lens, 8, 2, 128, 1, seed=111 + causal)
    probe = ctypes.c_int32(-1)
    monkeypatch.setattr(ops, "_PERSISTENT", False)
    with ops.launch_hooks(grid_probe=probe):
        want = _run(q, k, v, cu, cu, causal)
    ordinary = probe.value
    monkeypatch.setattr(ops, "_PERSISTENT", True)
    with ops.launch_hooks(grid_probe=probe, force_persistent=True):
        got = _run(q, k, v, cu, cu, causal)
    assert 0 < probe.value < ordinary
    assert torch.equal(got, want)
