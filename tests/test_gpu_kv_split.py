"""GPU: the exact split of the FP8-PV kv_lens family (``num_splits=``: a call of one query block as S key-range chunks -- pass 1 the chunk
maxima, pass 2 the seeded KVLEN kernels per chunk, the FP32 merge).

The route promises that every P is the P of the same call without ``num_splits``; only the FP32 summation order of O and l differs.  So
  1. every case is compared with the same call without the keyword at the bars of test_gpu_split_exact.py for "summation order only": 2 output
     ulps + 1e-5 max|o| element by element, rel-RMS <= 1e-3, LSE 1e-5 relative with -inf matching -inf -- plain random data and two key-magnitude
     profiles, rising along the sequence (the maximum moves in every chunk) and falling (later chunks' P are tiny against their seed);
  2. pass 1's chunk_max segment of the workspace is compared bit for bit with a numpy restatement in exact arithmetic (two shapes);
  3. one case per route is compared with the exact CPU oracle at the default routes' bar, 2e-3 max|ref| + one output ulp;
  4. the route that ran: grid_out is B * Hq * S, or B * Hkv * ceil(group / 4) * S packed, against the unsplit grid (on a tree without the feature
     the keyword falls into ``**kwargs`` and the grids are equal: this test fails there);
  5. padding behind a sample's length is never read by any of the three launches: the caller's rows NaN / 0x5A, and -- inside tests/fence.py's
     guarded allocator, both fills, five cases, gap rows -- the INT8 rows, k scale slots and V tiles the pre-pass leaves unwritten past len_b
     (the split workspace is one of the allocator's allocations);
  6. one graph capture replays with other lengths in the same tensor.

Lk = 1061 (17 tiles, the last ragged), S = 4 (T = 5: chunks of 5, 5, 5, 2 tiles), lengths 1061 / 700 / 320 / 321 / 1 / 0: full, mid-chunk, exactly
a chunk boundary, one key past it, one key, empty.  Also S = 2, 17 (one tile per chunk) and 16 (T = 2: trailing chunks past the tensor).
"""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import util
from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, core as sc, ops, quant as sq
    DEV = torch.device("cuda:0")

LK = 1061
LENS = (1061, 700, 320, 321, 1, 0)
STARTS = (1000, 77, -3, 300, 0, 5)          # unaligned; sample 2: rows in front of key 0; sample 5: an offset against no key
B = len(LENS)
F16, BF16 = torch.float16, torch.bfloat16
FP8 = lambda *a, **kw: sa.sageattn_qk_int8_pv_fp8_cuda(*a, **kw)
ROUTES = ("lens", "plain", "br", "qstart", "causal")


def _ints(values, dtype=torch.int32):
    return torch.tensor(list(values), dtype=dtype, device=DEV)


def _route_kw(route):
    if route == "lens":
        return dict(is_causal=False, kv_lens=_ints(LENS))
    if route == "plain":
        return dict(is_causal=False)
    if route == "br":
        return dict(is_causal=True, causal_align="bottom_right", kv_lens=_ints(LENS))
    if route == "qstart":
        return dict(is_causal=True, kv_lens=_ints(LENS), q_start=_ints(STARTS))
    assert route == "causal"                       # top-left, no offsets
    return dict(is_causal=True, kv_lens=_ints(LENS, torch.int64))


# (route, (Hq, Hkv), Lq, packed, D, dtype, layout, smooth_k, S, key profile): drawn sparingly -- every route at S 4 unpacked and packed, every
# S, every head pair, every Lq of both forms, every D / dtype / layout / smooth_k, both profiles on a non-causal and a causal route
CASES = [
    ("lens",   (8, 2), 1,   True,  128, BF16, "HND", True,  4,  "rand"),
    ("lens",   (4, 4), 33,  False, 64,  F16,  "NHD", False, 4,  "rand"),
    ("lens",   (6, 2), 5,   True,  64,  F16,  "HND", True,  17, "rise"),
    ("lens",   (5, 1), 128, False, 128, BF16, "NHD", False, 16, "fall"),
    ("lens",   (8, 2), 32,  True,  96,  F16,  "NHD", True,  2,  "fall"),
    ("plain",  (8, 2), 5,   True,  64,  BF16, "NHD", False, 4,  "rand"),
    ("plain",  (4, 4), 1,   False, 128, F16,  "HND", True,  16, "rise"),
    ("plain",  (6, 2), 128, False, 96,  BF16, "HND", True,  4,  "rand"),
    ("br",     (8, 2), 5,   True,  128, F16,  "NHD", True,  4,  "rand"),
    ("br",     (5, 1), 32,  True,  64,  BF16, "HND", False, 17, "fall"),
    ("br",     (4, 4), 128, False, 128, BF16, "HND", True,  4,  "rise"),
    ("br",     (6, 2), 1,   False, 64,  F16,  "NHD", False, 2,  "rand"),
    ("br",     (8, 2), 33,  False, 96,  BF16, "NHD", False, 16, "rand"),
    ("qstart", (6, 2), 32,  True,  128, BF16, "HND", False, 4,  "rand"),
    ("qstart", (8, 2), 33,  False, 64,  F16,  "HND", True,  4,  "fall"),
    ("qstart", (5, 1), 5,   True,  128, F16,  "NHD", True,  16, "rise"),
    ("qstart", (4, 4), 128, False, 64,  BF16, "NHD", False, 17, "rand"),
    ("causal", (8, 2), 32,  True,  64,  F16,  "HND", False, 4,  "rand"),
    ("causal", (6, 2), 128, False, 128, BF16, "NHD", True,  2,  "rand"),
    ("causal", (5, 1), 1,   True,  128, BF16, "HND", True,  17, "rand"),
]
IDS = [f"{r}-h{hq}_{hkv}-lq{lq}-{'pk' if pk else 'un'}-d{D}-{'f16' if dt == F16 else 'bf16'}-{lay}-{'sk' if sk else 'nosk'}-s{S}-{prof}"
       for r, (hq, hkv), lq, pk, D, dt, lay, sk, S, prof in CASES]
assert len(set(IDS)) == len(IDS)
assert {c[0] for c in CASES} == set(ROUTES) and {c[8] for c in CASES} == {2, 4, 16, 17} and {c[1] for c in CASES} == {(8, 2), (6, 2), (5, 1), (4, 4)}
assert {c[2] for c in CASES if c[3]} == {1, 5, 32} and {c[2] for c in CASES if not c[3]} == {1, 33, 128}
assert {(c[0], c[3]) for c in CASES if c[8] == 4} == {(r, p) for r in ROUTES for p in (False, True)} - {("causal", False)}
assert {c[4] for c in CASES} == {64, 128, 96} and {(c[5], c[6], c[7]) for c in CASES} == {(d, l, s) for d in (F16, BF16) for l in ("HND", "NHD") for s in (False, True)}
assert {(c[0] in ("lens", "plain"), c[9]) for c in CASES} >= {(nc, p) for nc in (False, True) for p in ("rise", "fall")}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _lay(t, layout):
    return t if layout == "HND" else t.transpose(1, 2).contiguous()


def _hnd(t, layout):
    return t if layout == "HND" else t.transpose(1, 2)


def _cut(t, b, n, layout):
    return (t[b:b + 1, :, :n] if layout == "HND" else t[b:b + 1, :n]).contiguous()


@functools.lru_cache(maxsize=None)
def _kv(hkv, D, dt, layout, profile="rand"):
    """Keys whose magnitude is flat, rises 64-fold along the sequence or falls 64-fold: rising, the row maximum moves in every chunk; falling,
    the first chunk holds it and later chunks' P are tiny against their seed, some rounding to zero."""
    g = torch.Generator().manual_seed(7 + D + hkv)
    k = torch.randn(B, hkv, LK, D, generator=g) + 0.25 * torch.randn(1, hkv, 1, D, generator=g)
    v = torch.randn(B, hkv, LK, D, generator=g)
    if profile != "rand":
        ramp = 8.0 ** torch.linspace(-1.0, 1.0, LK)
        k = k * (ramp if profile == "rise" else ramp.flip(0))[None, None, :, None]
    return tuple(_lay(t.to(dt).to(DEV), layout) for t in (k, v))


@functools.lru_cache(maxsize=None)
def _q(hq, lq, D, dt, layout):
    g = torch.Generator().manual_seed(1000 * hq + 10 * lq + D)
    return _lay(torch.randn(B, hq, lq, D, generator=g).to(dt).to(DEV), layout)


def _call(case, split, k=None, v=None, **more):
    route, (hq, hkv), lq, packed, D, dt, layout, smooth_k, S, prof = case
    k0, v0 = _kv(hkv, D, dt, layout, prof)
    kw = dict(_route_kw(route), **more)
    return FP8(_q(hq, lq, D, dt, layout), k0 if k is None else k, v0 if v is None else v, tensor_layout=layout, smooth_k=smooth_k, return_lse=True,
               pack_gqa=True if packed else None, num_splits=S if split else None, **kw)


@functools.lru_cache(maxsize=None)
def _unsplit(case):
    """The reference of a case: the same call without ``num_splits``.  Computed once, shared, never modified."""
    return _call(case, False)


def _ulp(x: np.ndarray, dt) -> np.ndarray:
    a = np.maximum(np.abs(x), 1e-30)
    u = 2.0 ** (np.floor(np.log2(a)) - (7 if dt == BF16 else 10))
    return np.maximum(u, 2.0 ** -24 if dt == F16 else 0.0)


def _o_distance(o, o0, dt):
    """The distance of o from the unsplit call's as fractions of the two bars: 2 output ulps + 1e-5 max|o| per element, rel-RMS 1e-3."""
    a, b = o.float().cpu().numpy(), o0.float().cpu().numpy()
    assert np.isfinite(a).all()
    m = float(np.abs(b).max())
    elem = float((np.abs(a - b) / (2 * _ulp(b, dt) + 1e-5 * m)).max())
    rms = float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30)) / 1e-3
    return elem, rms


def _distance(got, want, dt):
    """The largest distance of (o, lse) from the unsplit call's as fractions of the three bars (element, rel-RMS, LSE); -inf must match -inf."""
    elem, rms = _o_distance(got[0], want[0], dt)
    la, lb = got[1].cpu().numpy(), want[1].cpu().numpy()
    assert not np.isnan(la).any() and np.array_equal(np.isneginf(la), np.isneginf(lb)), "rows without a visible key differ"
    fin = np.isfinite(lb)
    lse = float((np.abs(la[fin] - lb[fin]) / (1e-5 * np.maximum(1.0, np.abs(lb[fin])))).max()) if fin.any() else 0.0
    return elem, rms, lse


# ---------------------------------------------------------------------------------------------- 1. against the call without num_splits
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_split_matches_the_unsplit_call(case):
    route, (hq, hkv), lq, packed, D, dt, layout, smooth_k, S, prof = case
    want = _unsplit(case)
    got = _call(case, True)
    torch.cuda.synchronize()
    assert got[0].shape == want[0].shape and got[0].dtype == dt and got[1].shape == (B, hq, lq)
    elem, rms, lse = _distance(got, want, dt)
    print(f"{IDS[CASES.index(case)]}: element {elem:.3f}, rel-RMS {rms:.3f}, lse {lse:.3f} of their bars")
    assert elem <= 1.0 and rms <= 1.0 and lse <= 1.0, (elem, rms, lse)
    # rows that see nothing: o = +0, lse = -inf
    empty = torch.isneginf(got[1])
    if route != "plain":
        assert bool(empty[5].all())                                  # the sample without keys
    o_rows = _hnd(got[0], layout)
    assert not bool(o_rows[empty].any()) and not bool(torch.signbit(o_rows[empty].float()).any())


def test_sageattn_forwards_the_keyword_and_auto_plans():
    case = CASES[0]
    route, (hq, hkv), lq, packed, D, dt, layout, smooth_k, S, prof = case
    k, v = _kv(hkv, D, dt, layout, prof)
    q = _q(hq, lq, D, dt, layout)
    kw = dict(tensor_layout=layout, return_lse=True, pack_gqa=True, **_route_kw(route))
    probe = ctypes.c_int32(-1)
    with ops.launch_hooks(grid_probe=probe):
        got = sa.sageattn(q, k, v, num_splits=4, **kw)
    assert probe.value == B * hkv * 4
    want = sa.sageattn(q, k, v, **kw)
    assert max(_distance(got, want, dt)) <= 1.0
    for auto in ("auto", 0):                                         # 17 tiles are below the auto plan's shortest key range: no split, today's bits
        assert sc._num_splits_plan(B, hq, hkv, lq, LK, True) == 0
        with ops.launch_hooks(grid_probe=probe):
            got = sa.sageattn(q, k, v, num_splits=auto, **kw)
        assert probe.value == B * hkv and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for off in (None, 1):                                            # today's call, bit for bit
        with ops.launch_hooks(grid_probe=probe):
            got = sa.sageattn(q, k, v, num_splits=off, **kw)
        assert probe.value == B * hkv and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_the_auto_plan_splits_a_long_key_range():
    """One sequence, 8192 keys, two packed workgroups: the plan takes 16 chunks of eight tiles, and the call is the unsplit one's."""
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(1, h, n, 64, generator=g).to(BF16).to(DEV) for h, n in ((8, 1), (2, 8192), (2, 8192)))
    lens = _ints((8000,))
    kw = dict(is_causal=True, causal_align="bottom_right", kv_lens=lens, pack_gqa=True, return_lse=True)
    assert sc._num_splits_plan(1, 8, 2, 1, 8192, True) == 16
    probe = ctypes.c_int32(-1)
    with ops.launch_hooks(grid_probe=probe):
        got = FP8(q, k, v, num_splits="auto", **kw)
    assert probe.value == 2 * 16
    assert max(_distance(got, FP8(q, k, v, **kw), BF16)) <= 1.0


# ---------------------------------------------------------------------------------------------- 2. pass 1 bit for bit
def _rne_f32(fr: Fraction) -> np.float32:
    """fr rounded once, to nearest even, to float32 (exact: the candidates around the float64 approximation are compared as fractions)."""
    x = np.float32(float(fr))
    cands = [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]
    return np.float32(min(cands, key=lambda c: (abs(Fraction(float(c)) - fr), int(np.array(c).view(np.uint32)) & 1)))


def _chunk_max_restated(q_int8, q_scale, k_int8, k_scale, S, lens, starts, sm_log2):
    """Pass 1 on numpy, as test_gpu_split_exact.py::chunk_max_restated, extended by the two masks: key < len_b and (``starts`` not None)
    key <= s_b + row, lengths and offsets clamped as the kernels clamp them; T = ceil(ceil(Lk / 64) / S).  [B, Hkv, S, group, Lq]."""
    nb, Hq, Lq, D = q_int8.shape
    Hkv, Lk = k_int8.shape[1], k_int8.shape[2]
    group, nt = Hq // Hkv, (Lk + 63) // 64
    T = (nt + S - 1) // S
    off = Fraction(float(np.float32(8.807)))
    sm = np.float32(sm_log2)
    out = np.full((nb, Hkv, S, group, Lq), -np.inf, dtype=np.float32)
    rows = np.arange(Lq)
    qslot = ((rows % 128) >> 5) * 8 + (rows & 7)
    for b in range(nb):
        n = max(0, min(int(lens[b]), Lk))
        s = None if starts is None else max(-Lq, min(int(starts[b]), Lk))
        for h in range(Hq):
            hk = h // group
            raw = q_int8[b, h].astype(np.int64) @ k_int8[b, hk, :n].astype(np.int64).T          # [Lq, n]: keys from len_b on are never touched
            for r in range(Lq):
                last = n - 1 if s is None else min(n - 1, s + r)
                qs = np.float32(q_scale[b, h, qslot[r]])
                for c in range(S):
                    best = -np.inf
                    for t in range(c * T, min((c + 1) * T, nt)):
                        for j in range(4):
                            keys = [64 * t + 8 * a + 2 * j + e for a in range(8) for e in range(2)]
                            vis = [x for x in keys if x <= last]
                            if not vis:
                                continue
                            u = np.float32(sm * np.float32(qs * np.float32(k_scale[b, hk, 4 * t + j])))
                            best = max(best, float(_rne_f32(Fraction(int(raw[r, vis].max())) * Fraction(float(u)) - off)))
                    out[b, hk, c, h - hk * group, r] = best
    return out


@pytest.mark.parametrize("causal,hq,hkv,lq,D,dt,S", [(False, 4, 2, 33, 64, F16, 4), (True, 6, 2, 5, 128, BF16, 4)], ids=["lens", "br_lq5"])
def test_pass1_chunk_maxima_are_bit_exact(causal, hq, hkv, lq, D, dt, S):
    """The C entry with a workspace of the test's own: its first segment against the restatement, every element written."""
    k, v = _kv(hkv, D, dt, "HND")
    q = _q(hq, lq, D, dt, "HND")
    lens = _ints(LENS)
    starts = (lens.clamp(0, LK) - lq).to(torch.int32) if causal else None
    _, _, k_int8, k_scale, v_image, v_scale, _ = sc._prepass_kv(q, k, v, "HND", "per_thread", 64, True, False, False, False, kv_lens=lens)
    q_int8, q_scale, _, _ = sq.per_thread_int8(q, k)
    sm_log2 = sc._sm_log2(D ** -0.5)
    nbytes = _cabi.kv_split_ws_bytes(B, hq, lq, D, S)
    ws = torch.full((nbytes // 4,), 7.0, dtype=torch.float32, device=DEV)
    o = torch.empty_like(q)
    lse = torch.empty((B, hq, lq), dtype=torch.float32, device=DEV)
    grid = ctypes.c_int32(-1)
    attr = _cabi.launch_attr(ws, grid_out=grid, q_start=starts, kv_split=S)
    _, _, _, _, q_sb, q_sh, q_sl = sq._dims(q, "HND")
    _, _, _, _, k_sb, k_sh, k_sl = sq._dims(k_int8, "HND")
    _, _, _, _, o_sb, o_sh, o_sl = sq._dims(o, "HND")
    code = 0 if dt == F16 else 1
    rc = _cabi.load().sage_attn_fused_q_pv_f8_kvlens(sq._p(q), sq._p(k_int8), sq._p(v_image), sq._p(o), sq._p(lse), sq._p(k_scale), sq._p(v_scale), None,
                                                     sq._p(lens), B, hq, hkv, lq, LK, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, o_sb, o_sh, o_sl,
                                                     int(causal), sm_log2, code, code, sq._stream(q), _cabi.attr_arg(attr))
    _cabi.check(rc, "sage_attn_fused_q_pv_f8_kvlens")
    torch.cuda.synchronize()
    assert grid.value == B * hq * S
    rows = B * hq * S * lq
    got = ws[:rows].cpu().numpy().reshape(B, hkv, S, hq // hkv, lq)
    want = _chunk_max_restated(q_int8.cpu().numpy(), q_scale.cpu().numpy(), k_int8.cpu().numpy(), k_scale.cpu().numpy(), S, LENS,
                               None if starts is None else starts.cpu().numpy(), sm_log2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    assert np.isneginf(got[5]).all() and np.isneginf(got[2, :, 1:]).sum() >= (S - 2) * hq * lq      # the empty sample; chunks from len 320 = 5 tiles on
    assert max(_o_distance(o, FP8(q, k, v, is_causal=causal, kv_lens=lens, q_start=starts), dt)) <= 1.0      # (and the call itself is the unsplit one's)


# ---------------------------------------------------------------------------------------------- 3. the exact CPU oracle
ORACLE_CASES = [CASES[0], CASES[5], CASES[8], CASES[14], CASES[17]]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[IDS[CASES.index(c)] for c in ORACLE_CASES])
def test_split_vs_oracle(oracle_mod, case):
    """One case per route, per sample against the exact CPU oracle on the sample's valid keys (the restatement of test_gpu_gqa_pack.py)."""
    from test_gpu_gqa_pack import _oracle_sample
    route, (hq, hkv), lq, packed, D, dt, layout, smooth_k, S, prof = case
    assert hkv == 2                                                   # (the oracle helper's LSE correction is written for two kv heads)
    code = 0 if dt == F16 else 1
    k, v = _kv(hkv, D, dt, layout, prof)
    q = _q(hq, lq, D, dt, layout)
    o, lse = _call(case, True)
    lens = (LK,) * B if route == "plain" else LENS
    starts = {"lens": None, "plain": None, "qstart": STARTS, "causal": (0,) * B}.get(route, tuple(n - lq for n in lens))
    for b, n in enumerate(lens):
        s = None if starts is None else max(-lq, min(starts[b], LK))
        qb, kb, vb = (_hnd(t, layout).contiguous() for t in (q[b:b + 1], _cut(k, b, n, layout), _cut(v, b, n, layout)))
        ref, lse_ref = _oracle_sample(oracle_mod, qb, kb, vb, code, D, smooth_k, s, 0)
        got, lgot = _hnd(o[b:b + 1], layout).float().cpu().numpy(), lse[b:b + 1].cpu().numpy()
        empty = np.isneginf(lse_ref)
        scale = float(np.abs(ref).max())
        err = float(np.abs(got - ref).max())
        lerr = float(np.abs(lgot[~empty] - lse_ref[~empty]).max()) if (~empty).any() else 0.0
        print(f"{route} sample {b} len {n} offset {s}: max|diff| {err:.3e} (bar {2e-3 * scale + util.out_ulp(scale, code):.3e}), lse {lerr:.3e}")
        assert np.isfinite(got).all() and np.array_equal(np.isneginf(lgot), empty), (b, n, s)
        assert not got[empty].any(), (b, n, s)
        assert err <= 2e-3 * scale + util.out_ulp(scale, code), (b, n, s)
        assert lerr <= 5e-3, (b, n, s)


# ---------------------------------------------------------------------------------------------- 4. the route that ran
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[9], CASES[12], CASES[15], CASES[18]],
                         ids=[IDS[i] for i in (0, 1, 9, 12, 15, 18)])
def test_the_split_route_ran(monkeypatch, case):
    """grid_out is pass 2's grid, S times the unsplit launch's, and the launch carried SAGE_ATTR_KV_SPLIT with the count in flags bits 16-23."""
    route, (hq, hkv), lq, packed, D, dt, layout, smooth_k, S, prof = case
    seen = []
    real = _cabi.launch_attr

    def spy(*a, **kw):
        attr = real(*a, **kw)
        seen.append(None if attr is None else int(attr.flags))
        return attr
    monkeypatch.setattr(_cabi, "launch_attr", spy)
    probe = ctypes.c_int32(-1)
    grids = {}
    for split in (True, False):
        del seen[:]
        probe.value = -1
        with ops.launch_hooks(grid_probe=probe):
            _call(case, split)
        torch.cuda.synchronize()
        assert len(seen) == 1 and seen[0] is not None, seen
        assert bool(seen[0] & _cabi.ATTR_KV_SPLIT) == split and (seen[0] >> _cabi.ATTR_KV_SPLIT_SHIFT) & 0xFF == (S if split else 0), (split, seen)
        grids[split] = probe.value
    unsplit = B * hkv * ((hq // hkv + 3) // 4) if packed else B * hq
    assert grids[False] == unsplit and grids[True] == unsplit * S, (grids, case)


# ---------------------------------------------------------------------------------------------- 5. padding
def _poisoned(t, lens, layout, byte):
    """``t`` with the rows from each sample's length on overwritten with ``byte``."""
    out = t.clone()
    raw = _hnd(out, layout).view(torch.int16)
    fill = int(np.array([byte, byte], dtype=np.uint8).view(np.int16)[0])
    for b, n in enumerate(lens):
        raw[b, :, max(0, min(n, raw.shape[2])):] = fill      # (raw.shape[2]: LK here, other padded lengths in the sweeps that import this)
    return out


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[9], CASES[14]], ids=[IDS[i] for i in (0, 3, 9, 14)])
def test_padding_is_never_read(case):
    """The CALLER's rows from len_b on hold NaN (0xFF) / 0x5A: the results are those of the clean tensors, bit for bit.  (This reaches the
    pre-pass and whatever read the caller's rows directly; the operands the three launches read -- INT8 K rows, k scale slots, V tiles -- are
    not formed from those rows: the kv_lens pre-pass leaves them unwritten past len_b.  They are poisoned in the fenced test below.)"""
    route, (hq, hkv), lq, packed, D, dt, layout, smooth_k, S, prof = case
    k, v = _kv(hkv, D, dt, layout, prof)
    want = _call(case, True)
    for fill in FILLS:
        got = _call(case, True, k=_poisoned(k, LENS, layout, fill), v=_poisoned(v, LENS, layout, fill))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"padding byte 0x{fill:02X}"


# packed bottom-right Lq 5; non-causal unpacked Lq 33 (pass 1's one-head-per-workgroup mapping); non-causal unpacked Lq 128 with chunks past the
# tensor; unaligned offsets, unpacked; non-causal packed Lq 1
FENCED = (8, 1, 3, 14, 0)


@pytest.mark.parametrize("case", [CASES[i] for i in FENCED], ids=[IDS[i] for i in FENCED])
def test_fenced_intermediates_past_the_lengths_are_never_read(case):
    """Inside the guarded allocator every allocation of the call starts out as the fill byte, so what the kv_lens pre-pass leaves unwritten
    past len_b -- INT8 K rows, k scale slots, V tiles, the scales of the empty sample -- is NaN (0xFF) or 0x5A in front of pass 1, pass 2 and
    the merge, and so is the split workspace before pass 1 and pass 2 fill it.  Both fills; inputs with gap rows behind every head; the
    result is the unfenced call's, bit for bit, and no guard is touched."""
    route, (hq, hkv), lq, packed, D, dt, layout, smooth_k, S, prof = case
    k, v = _kv(hkv, D, dt, layout, prof)
    q = _q(hq, lq, D, dt, layout)
    want = _call(case, True)
    for fill in FILLS:
        kp, vp = _poisoned(k, LENS, layout, fill), _poisoned(v, LENS, layout, fill)
        with Fence(fill) as f:
            rkw = {a: (f.input(b) if isinstance(b, torch.Tensor) else b) for a, b in _route_kw(route).items()}
            got = FP8(f.input(q, 3, layout), f.input(kp, 3, layout), f.input(vp, 3, layout), tensor_layout=layout, smooth_k=smooth_k, return_lse=True,
                      pack_gqa=True if packed else None, num_splits=S, **rkw)
            f.check()
            assert f.owns(got[0])
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"fill 0x{fill:02X}"


# ---------------------------------------------------------------------------------------------- 6. graph capture
def test_graph_capture_follows_the_lengths():
    """One capture on a single stream; kv_lens changed in place between replays: each replay equals the eager call on the new lengths."""
    hq, hkv, lq, D, dt, layout, S = 6, 2, 5, 128, F16, "HND", 4
    k, v = _kv(hkv, D, dt, layout)
    q = _q(hq, lq, D, dt, layout)
    lens = _ints(LENS)
    call = lambda n: FP8(q, k, v, tensor_layout=layout, is_causal=True, causal_align="bottom_right", return_lse=True, kv_lens=n, pack_gqa=True,
                         num_splits=S)
    call(lens)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(lens)
    torch.cuda.current_stream().wait_stream(s)
    probe = ctypes.c_int32(-1)
    with torch.cuda.graph(g):
        with ops.launch_hooks(grid_probe=probe):
            o, lse = call(lens)
    assert probe.value == B * hkv * S
    for values in ((17, 640, 0, 1061, 321, 5), (0, 0, 1061, 64, 320, 1), LENS):
        lens.copy_(_ints(values))
        g.replay()
        eager = call(_ints(values))
        torch.cuda.synchronize()
        assert torch.equal(o, eager[0]) and torch.equal(lse, eager[1]), f"replay with {values}"
