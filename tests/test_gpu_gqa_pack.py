"""GPU: the packed decode launch of the FP8-PV kv_lens kernels (``pack_gqa=True``: the query heads of a GQA group four to a workgroup, one
wave each over one shared K / V ring).

The route promises one thing: ``o`` and ``lse`` equal, bit for bit, those of the same call with ``pack_gqa=False``.  So
  1. every case is compared with ``torch.equal`` against the unpacked call -- on every route of the kernel family, for groups of 4, 3 (one idle
     wave), 8 (two blocks) and 5 (4 + 1: three idle waves), Lq 1 ... 32;
  2. the route that ran is checked (a keyword that was swallowed would pass 1.): the launch carried SAGE_ATTR_GQA_PACK and had
     ``B * Hkv * ceil(group / 4)`` workgroups, against ``B * Hq`` without the keyword;
  3. one case per route and Lq in {1, 16} is compared with the exact CPU oracle at the default routes' bar, ``2e-3 max|ref| + one output ulp``,
     LSE within 5e-3 (test_gpu_q_start.py::test_decode_shapes_vs_oracle; the window's left edge as the oracle's boolean mask);
  4. padding behind a sample's length is never read and nothing outside the outputs is written (NaN / 0x5A padding; groups 3 and 5 and the
     NHD layout inside tests/fence.py's guarded, poisoned allocator, with gap rows behind every head);
  5. one graph capture replays with other lengths in the same tensor.

B = 3, Hkv = 2, Lk = 640; lengths 640 / 333 / 0 (non-causal routes) and 640 / 333 / 1 (bottom-right ones); the padding rows of k / v hold
random data.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util
from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, ops, quant as sq
    DEV = torch.device("cuda:0")

B, HKV, LK = 3, 2, 640
LENS_NC, LENS_BR, STARTS = (640, 333, 0), (640, 333, 1), (601, 77, -3)
HEADS = ((8, 2), (6, 2), (16, 2), (10, 2))        # groups of 4, 3 (one idle wave), 8 (two blocks), 5 (4 + 1: three idle waves)
LQS = (1, 5, 16, 32)
F16, BF16 = torch.float16, torch.bfloat16
FP8 = lambda *a, **kw: sa.sageattn_qk_int8_pv_fp8_cuda(*a, **kw)
# the routes of the kernel family: non-causal lengths, no lengths at all, bottom-right with lengths, unaligned offsets (rows in front of key 0
# among them), a window under bottom-right -- and the causal kernel without offsets (top-left lengths), which none of the others reaches
ROUTES = ("lens", "plain", "br", "qstart", "window", "causal_lens")


def _ints(values, dtype=torch.int32):
    return torch.tensor(list(values), dtype=dtype, device=DEV)


def _route_kw(route):
    """The keywords of a route (fresh tensors on every call)."""
    if route == "lens":
        return dict(is_causal=False, kv_lens=_ints(LENS_NC))
    if route == "plain":
        return dict(is_causal=False)
    if route == "br":
        return dict(is_causal=True, causal_align="bottom_right", kv_lens=_ints(LENS_BR))
    if route == "br_empty":                       # a sample without keys under bottom-right: its offset is -Lq, no row sees a key
        return dict(is_causal=True, causal_align="bottom_right", kv_lens=_ints(LENS_NC))
    if route == "qstart":
        return dict(is_causal=True, kv_lens=_ints(LENS_BR), q_start=_ints(STARTS))
    if route == "window":
        return dict(is_causal=True, causal_align="bottom_right", kv_lens=_ints(LENS_BR), window_size=(100, 0))
    assert route == "causal_lens"
    return dict(is_causal=True, kv_lens=_ints(LENS_BR))


def _cases():
    """(route, (Hq, Hkv), Lq, D, dtype, layout, smooth_k): every route x every group twice, the other axes cycled at strides that do not
    divide each other -- a covering selection, not the product (the assertions below say what it covers)."""
    out = []
    for r, route in enumerate(ROUTES):
        for h, heads in enumerate(HEADS):
            for rep in range(2 if route != "causal_lens" else 1):
                n = len(out)
                out.append((route, heads, LQS[(h + r + 2 * rep + (r >> 2)) % 4], (64, 128, 96)[n % 3], (F16, BF16)[n % 2],
                            ("HND", "NHD")[(n // 3 + h) % 2], bool((n + r) % 2)))
    out.append(("br_empty", (6, 2), 5, 128, BF16, "HND", True))
    out.append(("br_empty", (8, 2), 32, 64, F16, "NHD", False))
    return out


CASES = _cases()
IDS = [f"{r}-h{hq}_{hkv}-lq{lq}-d{D}-{'f16' if dt == F16 else 'bf16'}-{lay}-{'sk' if sk else 'nosk'}" for r, (hq, hkv), lq, D, dt, lay, sk in CASES]
assert 40 <= len(CASES) <= 48 and len(set(IDS)) == len(IDS)
assert {(c[0], c[1]) for c in CASES} >= set(itertools.product(ROUTES, HEADS))
assert {(c[1], c[2]) for c in CASES} >= set(itertools.product(HEADS, LQS))          # every group at every row count
assert {(c[0], c[3]) for c in CASES} >= set(itertools.product(ROUTES[:5], (64, 128, 96)))
assert {(c[3], c[4]) for c in CASES} == set(itertools.product((64, 128, 96), (F16, BF16)))
assert {(c[3], c[5], c[6]) for c in CASES} >= set(itertools.product((64, 128), ("HND", "NHD"), (False, True)))
assert {(c[0], c[2]) for c in CASES} >= set(itertools.product(ROUTES[:5], LQS))
assert all({(c[0], c[i]) for c in CASES} >= set(itertools.product(ROUTES, vals)) for i, vals in ((4, (F16, BF16)), (5, ("HND", "NHD")), (6, (False, True))))


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
def _kv(D, dt, layout):
    g = torch.Generator().manual_seed(7 + D)
    k = (torch.randn(B, HKV, LK, D, generator=g) + torch.randn(1, HKV, 1, D, generator=g)).to(dt)
    v = torch.randn(B, HKV, LK, D, generator=g).to(dt)
    return tuple(_lay(t.to(DEV), layout) for t in (k, v))


@functools.lru_cache(maxsize=None)
def _q(hq, lq, D, dt, layout):
    g = torch.Generator().manual_seed(1000 * hq + 10 * lq + D)
    return _lay(torch.randn(B, hq, lq, D, generator=g).to(dt).to(DEV), layout)


def _same(a, b, what=""):
    assert torch.equal(a[0], b[0]), f"{what}: o differs in {int((a[0] != b[0]).sum())} of {a[0].numel()} elements"
    assert torch.equal(a[1], b[1]), f"{what}: lse differs in {int((a[1] != b[1]).sum())} of {a[1].numel()} rows"


@functools.lru_cache(maxsize=None)
def _unpacked(case):
    """The reference of a case: the same call with ``pack_gqa=False``.  Computed once, shared, never modified."""
    route, (hq, hkv), lq, D, dt, layout, smooth_k = case
    k, v = _kv(D, dt, layout)
    return FP8(_q(hq, lq, D, dt, layout), k, v, tensor_layout=layout, smooth_k=smooth_k, return_lse=True, pack_gqa=False, **_route_kw(route))


def _rows_without_keys(route, lq):
    """Query rows (per head, over the batch) that see no key."""
    if route in ("lens", "br_empty"):
        return lq                                               # the sample without keys
    if route in ("br", "window"):
        return max(0, lq - 1)                                   # one key: only the last row sees it
    if route == "qstart":
        return min(lq, 3)                                       # offset -3 against one key: rows 0 .. 2 stand in front of key 0
    return 0


# ---------------------------------------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_packed_equals_unpacked_bit_for_bit(case):
    route, (hq, hkv), lq, D, dt, layout, smooth_k = case
    k, v = _kv(D, dt, layout)
    q = _q(hq, lq, D, dt, layout)
    want = _unpacked(case)
    got = FP8(q, k, v, tensor_layout=layout, smooth_k=smooth_k, return_lse=True, pack_gqa=True, **_route_kw(route))
    assert got[0].shape == q.shape and got[0].dtype == dt and got[1].shape == (B, hq, lq)
    _same(got, want, IDS[CASES.index(case)])
    # rows that see nothing: o = +0 and lse = -inf, never NaN -- in both launches
    o, lse = got[0].float(), got[1]
    assert not bool(torch.isnan(o).any()) and not bool(torch.isnan(lse).any())
    empty = torch.isneginf(lse)
    assert int(empty.sum()) == hq * _rows_without_keys(route, lq), (int(empty.sum()), route, lq)
    o_rows = _hnd(got[0], layout)
    assert not bool(o_rows[empty].any()) and not bool(torch.signbit(o_rows[empty].float()).any())


# ---------------------------------------------------------------------------------------------- 2. the route that ran
@pytest.mark.parametrize("heads", HEADS, ids=[f"h{a}_{b}" for a, b in HEADS])
@pytest.mark.parametrize("route", ROUTES)
def test_the_packed_route_ran(monkeypatch, route, heads):
    """The launch carries SAGE_ATTR_GQA_PACK and has B * Hkv * ceil(group / 4) workgroups; off, no flag and B * Hq.  (On a library without the
    feature the keyword falls into ``**kwargs``: no flag, B * Hq workgroups -- this test fails there.)"""
    hq, hkv = heads
    lq, D, dt, layout = 5, 64, F16, "HND"
    k, v = _kv(D, dt, layout)
    q = _q(hq, lq, D, dt, layout)
    seen = []
    real = _cabi.launch_attr

    def spy(*a, **kw):
        attr = real(*a, **kw)
        seen.append((dict(kw), None if attr is None else int(attr.flags)))
        return attr
    monkeypatch.setattr(_cabi, "launch_attr", spy)
    probe = ctypes.c_int32(-1)
    grids = {}
    for on in (True, False, None):
        del seen[:]
        probe.value = -1
        with ops.launch_hooks(grid_probe=probe):
            FP8(q, k, v, tensor_layout=layout, return_lse=True, pack_gqa=on, **_route_kw(route))
        torch.cuda.synchronize()
        assert len(seen) == 1, seen                                       # one attention launch
        kw, flags = seen[0]
        assert flags is not None and bool(flags & _cabi.ATTR_GQA_PACK) == bool(on) and bool(kw.get("gqa_pack")) == bool(on), (on, seen)
        grids[on] = probe.value
    group = hq // hkv
    assert grids[True] == B * hkv * ((group + 3) // 4), (grids, heads)
    assert grids[False] == grids[None] == B * hq, (grids, heads)


def test_sageattn_forwards_the_keyword():
    hq, lq, D, dt, layout = 8, 16, 128, BF16, "HND"
    k, v = _kv(D, dt, layout)
    q = _q(hq, lq, D, dt, layout)
    kw = dict(tensor_layout=layout, is_causal=True, return_lse=True, kv_lens=_ints(LENS_BR), causal_align="bottom_right")
    probe = ctypes.c_int32(-1)
    with ops.launch_hooks(grid_probe=probe):
        got = sa.sageattn(q, k, v, pack_gqa=True, **kw)
    assert probe.value == B * HKV
    _same(got, sa.sageattn(q, k, v, **kw), "sageattn")
    _same(got, FP8(q, k, v, pv_accum_dtype="fp32+fp32", pack_gqa=True, **kw), "sageattn is the FP8 entry point with fp32+fp32")


# ---------------------------------------------------------------------------------------------- 3. the exact CPU oracle
def _lse_post(oracle, lse, aux, qb, code, D, hq, smooth_k, rows):
    """sageattn_dense's own LSE post-processing (natural log; smooth_k: + q . km * sm_scale, the product rounded to the input dtype)."""
    lse = lse / np.float32(oracle.LOG2E)
    if smooth_k:
        kind = "f16" if code == 0 else "bf16"
        qf = oracle.to_f32(util.bits(qb if D in (64, 128) else F.pad(qb, (0, 128 - D))), code)
        kmf = np.repeat(oracle.to_f32(aux["km"], code), hq // HKV, axis=1)
        corr = oracle.to_f32(oracle.convert(np.einsum("bhld,bhd->bhl", qf, kmf), kind), code)
        lse = lse + corr[:, :, rows] * np.float32(1.0 / (D ** 0.5))
    return lse


def _oracle_sample(oracle, qb, kb, vb, code, D, smooth_k, s, W):
    """Reference o (float32 [1, Hq, lq, D]) and lse of one sample.  ``s`` None: non-causal.  Else row i sees key j iff j <= s + i (s already
    clamped to [-lq, Lk]) and, with a window ``W`` > 0, j > s + i - W: the shift restated by padding -- zero rows in front of q8 for a positive
    offset, rows dropped for a negative one -- the window's left edge as the oracle's boolean mask.  Rows that see nothing: exactly 0 / -inf."""
    hq, lq, n = qb.shape[1], qb.shape[2], kb.shape[2]
    o_ref, lse_ref = np.zeros((1, hq, lq, D), np.float32), np.full((1, hq, lq), -np.inf, np.float32)
    drop = max(0, -s) if s is not None else 0
    if n == 0 or drop >= lq:
        return o_ref, lse_ref
    km = util.bits(sq.channel_mean(kb if D in (64, 128) else F.pad(kb, (0, 128 - D)))) if smooth_k else None
    o, lse, aux = oracle.sageattn_dense(util.bits(qb), util.bits(kb), util.bits(vb), code, is_causal=s is not None, pv="f8",
                                        qk_quant_gran="per_thread", return_lse=True, km=km, smooth_k=smooth_k, fp8_scores="exact")
    if s is None:
        return util.f32(o, code)[..., :D], lse
    q8, gq = aux["q8"], aux["gq"]
    front = max(0, s)
    q8s = np.ascontiguousarray(np.concatenate([np.zeros(q8.shape[:2] + (front, q8.shape[3]), np.int8), q8[:, :, drop:]], axis=2))
    gqs = np.concatenate([np.zeros(front, np.int32), gq[drop:]])
    mask = None
    if W:
        rows, keys = np.arange(q8s.shape[2])[:, None], np.arange(n)[None, :]
        mask = (keys <= rows) & (keys > rows - W)
        mask[:front] = True                                 # (the padding rows: whatever, they are cut off below)
    o, lse = oracle.attn(q8s, aux["k8"], aux["v8"], aux["qs"], gqs, aux["ks"], aux["gk"], causal=mask is None, c=aux["c"],
                         pv_mode=oracle.PV_F8_TWO_LEVEL, out_dtype=code, v_scale=aux["vs"], return_lse=True, score_mode=oracle.SCORES_EXACT,
                         mask_bool=mask)
    o_ref[:, :, drop:] = util.f32(o, code)[:, :, front:, :D]
    lse_ref[:, :, drop:] = _lse_post(oracle, lse[:, :, front:], aux, qb, code, D, hq, smooth_k, slice(drop, None))
    return o_ref, lse_ref


ORACLE_CASES = [(route, lq, *((128, BF16, "HND", False) if (i + j) % 2 == 0 else (64, F16, "NHD", True)))
                for i, route in enumerate(ROUTES) for j, lq in enumerate((1, 16))]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[f"{c[0]}-lq{c[1]}-d{c[2]}-{c[4]}-{'sk' if c[5] else 'nosk'}" for c in ORACLE_CASES])
def test_packed_vs_oracle(oracle_mod, case):
    """Group 4, Lq 1 and 16, every route, per sample against the exact CPU oracle on the sample's valid keys."""
    route, lq, D, dt, layout, smooth_k = case
    hq, code = 8, 0 if dt == F16 else 1
    k, v = _kv(D, dt, layout)
    q = _q(hq, lq, D, dt, layout)
    o, lse = FP8(q, k, v, tensor_layout=layout, smooth_k=smooth_k, return_lse=True, pack_gqa=True, **_route_kw(route))
    lens = {"lens": LENS_NC, "plain": (LK,) * B}.get(route, LENS_BR)
    starts = {"lens": None, "plain": None, "qstart": STARTS, "causal_lens": (0,) * B}.get(route, tuple(n - lq for n in lens))
    for b, n in enumerate(lens):
        s = None if starts is None else max(-lq, min(starts[b], LK))
        qb, kb, vb = (_hnd(t, layout).contiguous() for t in (q[b:b + 1], _cut(k, b, n, layout), _cut(v, b, n, layout)))
        ref, lse_ref = _oracle_sample(oracle_mod, qb, kb, vb, code, D, smooth_k, s, 101 if route == "window" else 0)
        got, lgot = _hnd(o[b:b + 1], layout).float().cpu().numpy(), lse[b:b + 1].cpu().numpy()
        empty = np.isneginf(lse_ref)
        scale = float(np.abs(ref).max())
        err = float(np.abs(got - ref).max())
        lerr = float(np.abs(lgot[~empty] - lse_ref[~empty]).max()) if (~empty).any() else 0.0
        print(f"{route} sample {b} len {n} offset {s}: max|diff| {err:.3e} (bar {2e-3 * scale + util.out_ulp(scale, code):.3e}), lse {lerr:.3e}, "
              f"{int(empty.sum())} empty rows")
        assert np.isfinite(got).all() and not np.isnan(lgot).any(), (b, n, s)
        assert np.array_equal(np.isneginf(lgot), empty), (b, n, s)
        assert not got[empty].any() and not np.signbit(got[empty]).any(), (b, n, s)
        assert err <= 2e-3 * scale + util.out_ulp(scale, code), (b, n, s)
        assert lerr <= 5e-3, (b, n, s)


# ---------------------------------------------------------------------------------------------- 4. padding and neighbours
def _poisoned(t, lens, layout, byte):
    """``t`` with the rows from each sample's length on overwritten with ``byte``."""
    out = t.clone()
    raw = _hnd(out, layout).view(torch.int16)
    fill = int(np.array([byte, byte], dtype=np.uint8).view(np.int16)[0])
    for b, n in enumerate(lens):
        raw[b, :, max(0, min(n, LK)):] = fill
    return out


# group 3 (one idle wave), group 5 (three idle waves in the second block), and the NHD layout (head stride D: a wrong head index lands in the
# neighbouring head's rows, not past the tensor)
FENCED = [("lens", (6, 2), 16, 128, F16, "HND", True), ("br", (10, 2), 5, 64, BF16, "HND", False), ("window", (6, 2), 32, 128, BF16, "NHD", True)]


def test_padding_is_never_read_and_neighbours_are_never_written():
    for case in FENCED:
        route, (hq, hkv), lq, D, dt, layout, smooth_k = case
        k, v = _kv(D, dt, layout)
        q = _q(hq, lq, D, dt, layout)
        lens = LENS_NC if route == "lens" else LENS_BR
        kw = dict(tensor_layout=layout, smooth_k=smooth_k, return_lse=True, pack_gqa=True)
        ref = _unpacked(case)
        for fill in FILLS:
            kp, vp = _poisoned(k, lens, layout, fill), _poisoned(v, lens, layout, fill)
            _same(FP8(q, kp, vp, **kw, **_route_kw(route)), ref, f"{route}: padding byte 0x{fill:02X}")
            with Fence(fill) as f:
                rkw = {a: (f.input(b) if isinstance(b, torch.Tensor) else b) for a, b in _route_kw(route).items()}
                got = FP8(f.input(q, 3, layout), f.input(kp, 3, layout), f.input(vp, 3, layout), **kw, **rkw)
                f.check()
                _same(got, ref, f"{route}: fill 0x{fill:02X}, fenced, gap rows")
                assert f.owns(got[0])


# ---------------------------------------------------------------------------------------------- 5. graph capture
def test_graph_capture_follows_the_lengths():
    """One capture on a single stream; kv_lens changed in place between replays: each replay equals the eager call on the new lengths."""
    hq, lq, D, dt, layout = 10, 16, 128, F16, "HND"
    k, v = _kv(D, dt, layout)
    q = _q(hq, lq, D, dt, layout)
    lens = _ints(LENS_BR)
    call = lambda n: FP8(q, k, v, tensor_layout=layout, is_causal=True, causal_align="bottom_right", return_lse=True, kv_lens=n, pack_gqa=True)
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
    assert probe.value == B * HKV * 2                                    # group 5: two blocks per kv head
    for values in ((17, 640, 0), (512, 1, 333), LENS_BR):
        lens.copy_(_ints(values))
        g.replay()
        eager = call(_ints(values))
        torch.cuda.synchronize()
        _same((o, lse), eager, f"replay with {values}")
        _same(eager, FP8(q, k, v, tensor_layout=layout, is_causal=True, causal_align="bottom_right", return_lse=True, kv_lens=_ints(values)),
              f"unpacked, {values}")
