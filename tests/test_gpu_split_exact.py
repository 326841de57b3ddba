"""GPU: the exact split-KV route of sageattn_qk_int8_pv_fp8_cuda (``split_kv_exact=True``).

  * pass 1 (sage_split_exact_chunk_max) writes, bit for bit, the chunk maxima restated here from per_thread_int8's Q / K bits and scales,
    the fma and its one rounding to float32 done in exact arithmetic;
  * the route against the UNSPLIT call (split_kv=0) on the same inputs: every P is the same, so only the FP32 summation order of O and l
    differs -- within 2 output ulps element by element, 1e-3 rel-RMS, 1e-5 relative in the LSE (the inexact split_kv misses this by ~30x);
  * against the exact unsplit oracle at the default routes' bar; the route that ran; HIP-graph capture.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import util

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import oracle
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


def _qkv(B, Hq, Hkv, Lq, Lk, D, dt, seed, qk_mul=1.0, v_mul=1.0, layout="HND"):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Hq, Lq, D, generator=g) * qk_mul).to(_tdt(dt))
    k = ((torch.randn(B, Hkv, Lk, D, generator=g) + 0.5) * qk_mul).to(_tdt(dt))
    v = (torch.randn(B, Hkv, Lk, D, generator=g) * v_mul).to(_tdt(dt))
    if layout == "NHD":
        return tuple(t.transpose(1, 2).contiguous().to(DEV) for t in (q, k, v))
    return tuple(t.to(DEV) for t in (q, k, v))


def _hnd(t, layout):
    return t if layout == "HND" else t.transpose(1, 2)


# ------------------------------------------------------------------------------------------------ pass 1
def _rne_f32(fr: Fraction) -> np.float32:
    """fr rounded once, to nearest even, to float32 (exact: the candidates around the float64 approximation are compared as fractions)."""
    x = np.float32(float(fr))
    cands = [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - fr), int(np.array(c).view(np.uint32)) & 1))
    return np.float32(best)


def chunk_max_restated(q_int8, q_scale, k_int8, k_scale, Lk, S, causal, sm_log2):
    """Pass 1 on numpy: per (b, hq, row, chunk) the maximum over the chunk's k scale groups of
    RNE_f32(max visible raw score * (sm * (q_scale * k_scale)) - f32(8.807)); -inf where no key is visible.  [B, Hkv, S, group, Lq]."""
    B, Hq, Lq, D = q_int8.shape
    Hkv = k_int8.shape[1]
    group, ntw = Hq // Hkv, Lk // 64
    tpc = ntw // S
    off = Fraction(float(np.float32(8.807)))
    sm = np.float32(sm_log2)
    out = np.full((B, Hkv, S, group, Lq), -np.inf, dtype=np.float32)
    rows = np.arange(Lq)
    qslot = (rows // 128) * 32 + ((rows % 128) >> 5) * 8 + (rows & 7)
    for b in range(B):
        for h in range(Hq):
            hk = h // group
            raw = q_int8[b, h].astype(np.int64) @ k_int8[b, hk, :ntw * 64].astype(np.int64).T     # [Lq, ntw*64]
            keys = np.arange(ntw * 64)
            vis = np.ones_like(raw, dtype=bool) if not causal else keys[None, :] <= rows[:, None]
            masked = np.where(vis, raw, np.iinfo(np.int64).min)
            grp = masked.reshape(Lq, ntw, 8, 8)                     # (row, tile, key / 8, key % 8): scale group j = (key % 8) // 2
            for r in range(Lq):
                qs = np.float32(q_scale[b, h, qslot[r]])
                for c in range(S):
                    best = -np.inf
                    for t in range(c * tpc, (c + 1) * tpc):
                        for j in range(4):
                            mx = int(grp[r, t, :, 2 * j:2 * j + 2].max())
                            if mx == np.iinfo(np.int64).min:
                                continue
                            u = np.float32(sm * np.float32(qs * np.float32(k_scale[b, hk, 4 * t + j])))
                            val = _rne_f32(Fraction(mx) * Fraction(float(u)) - off)
                            best = max(best, float(val))
                    out[b, hk, c, h - hk * group, r] = best
    return out


@pytest.mark.parametrize("B,Hq,Hkv,Lq,Lk,D,S,causal,dt", [
    (1, 2, 1, 384, 384, 128, 2, True, 0),          # a chunk boundary through a 128-row block
    (1, 2, 2, 960, 960, 64, 5, True, 1),           # odd tile counts per chunk
    (1, 4, 1, 130, 2048 + 77, 128, 3, False, 1),   # GQA, ragged key range (pass 1 covers the 33 whole tiles)
    (2, 2, 1, 64, 1024, 64, 2, False, 0),
])
def test_pass1_chunk_maxima_are_bit_exact(B, Hq, Hkv, Lq, Lk, D, S, causal, dt):
    q, k, _ = _qkv(B, Hq, Hkv, Lq, Lk, D, dt, seed=Lq + Lk + D)
    q_int8, q_scale, k_int8, k_scale = sq.per_thread_int8(q, k)
    sm_log2 = sc._sm_log2(D ** -0.5)
    out = torch.full((B, Hq * S, Lq), 7.0, dtype=torch.float32, device=DEV)
    _, _, _, _, q_sb, q_sh, q_sl = sq._dims(q, "HND")
    _, _, _, _, k_sb, k_sh, k_sl = sq._dims(k_int8, "HND")
    rc = _cabi.load().sage_split_exact_chunk_max(sq._p(q), sq._p(k_int8), sq._p(k_scale), sq._p(out), B, Hq, Hkv, S, Lq, Lk, D,
                                                 q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, int(causal), sm_log2, dt, sq._stream(q))
    _cabi.check(rc, "sage_split_exact_chunk_max")
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(B, Hkv, S, Hq // Hkv, Lq)
    want = chunk_max_restated(q_int8.cpu().numpy(), q_scale.cpu().numpy(), k_int8.cpu().numpy(), k_scale.cpu().numpy(), Lk, S, causal, sm_log2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    if causal:
        assert np.isneginf(got).any()              # chunks behind a row's diagonal


# ------------------------------------------------------------------------------------------------ the route against the unsplit call
def _ulp(x: np.ndarray, dt: int) -> np.ndarray:
    a = np.maximum(np.abs(x), 1e-30)
    u = 2.0 ** (np.floor(np.log2(a)) - (7 if dt == 1 else 10))
    return np.maximum(u, 2.0 ** -24 if dt == 0 else 0.0)


def _run(q, k, v, layout, causal, **kw):
    return sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, tensor_layout=layout, is_causal=causal, pv_accum_dtype=kw.pop("accum", "fp32+fp32"),
                                           return_lse=True, **kw)


def _assert_matches_unsplit(o, lse, o0, lse0, dt, desc):
    a, b = o.float().cpu().numpy(), o0.float().cpu().numpy()
    assert np.isfinite(a).all(), desc
    m = float(np.abs(b).max())
    bad = np.abs(a - b) > 2 * _ulp(b, dt) + 1e-5 * m
    assert not bad.any(), (desc, int(bad.sum()), float(np.abs(a - b).max()), m)
    rel_rms = float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))
    assert rel_rms <= 1e-3, (desc, rel_rms)
    la, lb = lse.cpu().numpy(), lse0.cpu().numpy()
    assert np.all(np.abs(la - lb) <= 1e-5 * np.maximum(1.0, np.abs(lb))), (desc, float(np.abs(la - lb).max()))


CASES = [
    # B, Hq, Hkv, Lq, Lk, D, dt, layout, causal, split_kv, qk_mul, v_mul
    (1, 4, 4, 1, 8192, 128, 1, "HND", False, None, 1.0, 1.0),        # decode-like, auto plan
    (1, 4, 4, 128, 8192, 128, 0, "HND", False, None, 1.0, 1.0),
    (1, 8, 2, 16, 8192, 128, 1, "NHD", False, 4, 1.0, 1.0),           # GQA, explicit S
    (1, 4, 1, 100, 8192 + 77, 64, 0, "HND", False, None, 1.0, 1.0),   # ragged key range: tail chunk
    (1, 2, 2, 33, 4096 + 1, 128, 1, "NHD", False, 8, 1.0, 1.0),       # one key in the tail
    (1, 2, 2, 384, 384, 128, 0, "HND", True, 2, 1.0, 1.0),            # causal, a chunk boundary through a 128-row block
    (1, 2, 1, 960, 960, 64, 1, "NHD", True, 5, 1.0, 1.0),             # causal, odd tile counts
    (2, 4, 2, 1000, 1000, 128, 1, "HND", True, 3, 1.0, 1.0),          # causal + ragged tail (15 whole tiles in 3 chunks + 40 keys)
    (1, 4, 4, 64, 8192, 128, 1, "HND", False, 8, 30.0, 1.0e5),        # large magnitudes (bf16 values above fp16's range)
    (1, 4, 2, 128, 4096, 96, 0, "HND", False, 4, 1.0, 1.0),           # padded head dim
]


@pytest.mark.parametrize("case", CASES, ids=[f"c{i}" for i in range(len(CASES))])
def test_exact_split_matches_the_unsplit_call(case, monkeypatch):
    B, Hq, Hkv, Lq, Lk, D, dt, layout, causal, split, qk_mul, v_mul = case
    q, k, v = _qkv(B, Hq, Hkv, Lq, Lk, D, dt, seed=sum(case[:6]), qk_mul=qk_mul, v_mul=v_mul, layout=layout)
    o0, lse0 = _run(q, k, v, layout, causal, split_kv=0)
    calls = {"exact": 0, "split": 0, "unsplit": 0}
    for name, key in (("_attn_fused_q_split_exact", "exact"), ("_attn_fused_q_split", "split"), ("_attn_fused_q", "unsplit")):
        fn = getattr(sc, name)
        monkeypatch.setattr(sc, name, lambda *a, _fn=fn, _k=key, **kw: (calls.__setitem__(_k, calls[_k] + 1), _fn(*a, **kw))[1])
    o, lse = _run(q, k, v, layout, causal, split_kv_exact=True, split_kv=split, accum="fp32+fp16" if dt == 1 else "fp32+fp32")
    torch.cuda.synchronize()
    assert calls == {"exact": 1, "split": 0, "unsplit": 0}, calls
    _assert_matches_unsplit(o, lse, o0, lse0, dt, case)


def test_smooth_k_lse_and_v_mean_free_route():
    """smooth_k=False and the LSE correction of smooth_k=True (q . km added on the host) both agree with the unsplit call."""
    q, k, v = _qkv(1, 4, 2, 128, 4096 + 5, 128, 0, seed=11)
    for smooth in (False, True):
        o0, lse0 = _run(q, k, v, "HND", False, split_kv=0, smooth_k=smooth)
        o, lse = _run(q, k, v, "HND", False, split_kv_exact=True, split_kv=4, smooth_k=smooth)
        _assert_matches_unsplit(o, lse, o0, lse0, 0, smooth)


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5], CASES[8]], ids=["decode128", "ragged", "causal384", "large"])
def test_exact_split_meets_the_unsplit_oracle(case):
    B, Hq, Hkv, Lq, Lk, D, dt, layout, causal, split, qk_mul, v_mul = case
    q, k, v = _qkv(B, Hq, Hkv, Lq, Lk, D, dt, seed=sum(case[:6]), qk_mul=qk_mul, v_mul=v_mul, layout=layout)
    o = sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, tensor_layout=layout, is_causal=causal, pv_accum_dtype="fp32+fp32",
                                        split_kv_exact=True, split_kv=split)
    torch.cuda.synchronize()
    qh, kh, vh = (_hnd(t, layout).cpu() for t in (q, k, v))
    km = util.bits(sq.channel_mean(_hnd(k, layout).contiguous()))
    ref, _, _ = oracle.sageattn_dense(util.bits(qh), util.bits(kh), util.bits(vh), dt, is_causal=causal, pv="f8",
                                      qk_quant_gran="per_thread", km=km, fp8_scores="exact")
    ref = util.f32(ref, dt)
    got = _hnd(o, layout).float().cpu().numpy()
    scale = float(np.abs(ref).max())
    assert float(np.abs(got - ref).max()) <= 2e-3 * scale + util.out_ulp(scale, dt), (case, float(np.abs(got - ref).max()), scale)


def test_auto_plan_splits_decode_and_not_a_full_chip_shape():
    assert sc._split_exact_plan(1, 32, 128, 32768, False, None) >= 2                 # bench decode_like
    assert sc._split_exact_plan(1, 32, 128, 32768 + 77, False, "auto") >= 2          # ragged: the whole tiles are planned
    assert sc._split_exact_plan(2, 32, 8192, 8192, False, None) == 0                 # fills the chip already
    assert sc._split_exact_plan(1, 32, 128, 32768, True, None) == 0                  # causal: on request only


def test_exact_split_is_graph_capturable():
    """No host synchronisation and no data-dependent host decision: one capture on a single stream replays bit-identically to eager."""
    q, k, v = _qkv(1, 8, 2, 16, 8192 + 77, 128, 1, seed=3)
    call = lambda: sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, pv_accum_dtype="fp32+fp32", split_kv_exact=True)
    want = call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        o_graph = call()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o_graph, want)
