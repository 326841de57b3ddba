"""GPU: the sliding window of the packed FP8-PV route,
``sageattn_qk_int8_pv_fp8_varlen(causal_align="bottom_right", window_size=(W - 1, 0))``.

With ``s_b = Lk_b - Lq_b``, row i of sequence b attends to key j of that sequence iff ``s_b + i - W < j <= s_b + i`` and ``0 <= j < Lk_b``.
References:
  * ``tests/ref_varlen_window.py``, the packed FP8 arithmetic with a visibility predicate (pinned to the C oracle's packed causal path by
    tests/test_varlen_window_host.py), at the bar of the windowed routes: ``2e-3 max|ref| + 2 output ulps``, LSE within 5e-3, rows that see
    nothing exactly ``+0`` / ``-inf`` by closed form;
  * bit identities: a window that cuts no row against the call without the keyword; the two work-list routes; the ticket launch against the
    ordinary one; the route switches; operands in front of every sequence's first requested key poisoned; the run inside the fenced
    allocator.

BATCH, one packed call (GQA 4 / 2, D 64 and 128, fp16 and bf16), with W in {1, 100, 192, 448}:
  (448, 448) interior blocks: start behind key 0, head tiles, diagonal      (128, 568) offset 440: three general diagonal tiles
  (128, 1024) aligned offset: head + steady + pipelined diagonal tiles after kc0 > 0      (1, 1000) decode      (1, 50) decode with W > Lk
  (5, 700) verification      (300, 130) rows in front of key 0 sharing a block with rows that see keys      (7, 1) a lone key
  (64, 0) no keys      (0, 200) no rows      (128, 128) one full tile pair, Lq = Lk
(tests/test_varlen_window_host.py::test_loop_bounds_of_the_tested_batch holds the tiles they reach.)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import util
import ref_varlen_window as rvw
from fence import FILLS, Fence
from test_gpu_varlen_br import _call, _inputs, _km_of_call, _run, _same

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi, core as sc, ops
    DEV = torch.device("cuda:0")

BATCH = ((448, 448), (128, 568), (128, 1024), (1, 1000), (1, 50), (5, 700), (300, 130), (7, 1), (64, 0), (0, 200), (128, 128))
WINDOWS = (1, 100, 192, 448)
SQUARE = (1, 63, 64, 0, 65, 127, 129, 448, 1000)
GRID = [(64, 0), (64, 1), (128, 0), (128, 1)]
IDS = [f"d{D}-{'f16' if dt == 0 else 'bf16'}" for D, dt in GRID]
HQ, HKV = 4, 2
BR = dict(is_causal=True, causal_align="bottom_right")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _win(W):
    return dict(BR, window_size=(W - 1, 0))


def _batch_inputs(D, dt):
    return _inputs(BATCH, HQ, HKV, D, dt, 61 + D + dt)


@functools.lru_cache(maxsize=None)
def _batch_run(D, dt, W):
    """BATCH through the default route with the LSE: (o, lse) on the device.  Shared by the reference, identity, poison and fence cases."""
    return _run(_batch_inputs(D, dt), return_lse=True, **_win(W))


def _check_vs_reference(O, ins, dt, W, o, lse, km, tag):
    """Every sequence: max|diff| <= 2e-3 max|ref| + 2 output ulps at max|ref|; LSE within 5e-3; rows that see nothing exactly +0 / -inf, where
    the closed form says.  Returns the largest distance to the reference relative to its bar."""
    q, k, v, cu_q, cu_k = ins
    ref_bits, lse_ref = rvw.ref_f8_varlen_window(O, util.bits(q), util.bits(k), util.bits(v), dt, cu_q.numpy(), cu_k.numpy(), W, km=km,
                                                 return_lse=True)
    ref, got, lgot = util.f32(ref_bits, dt), o.float().cpu().numpy(), lse.cpu().numpy()
    assert not np.isnan(got).any() and np.isfinite(got).all() and not np.isnan(lgot).any() and not (lgot == np.inf).any(), tag
    empty = np.isneginf(lse_ref)
    assert np.array_equal(np.isneginf(lgot), empty), tag
    worst = 0.0
    for b in range(len(cu_q) - 1):
        s, e = int(cu_q[b]), int(cu_q[b + 1])
        lq, lk = e - s, int(cu_k[b + 1] - cu_k[b])
        if lq == 0:
            continue
        none = rvw.rows_without_keys(lq, lk, W)
        assert empty[:, s:e].sum() == q.shape[1] * none and empty[:, s:s + none].all(), (tag, b)
        assert not got[s:s + none].any() and not np.signbit(got[s:s + none]).any(), (tag, b)            # +0, not merely small
        scale = float(np.abs(ref[s:e]).max())
        bar = 2e-3 * scale + 2 * util.out_ulp(scale, dt)
        err = float(np.abs(got[s:e] - ref[s:e]).max())
        seen = ~empty[:, s:e]
        lerr = float(np.abs(lgot[:, s:e][seen] - lse_ref[:, s:e][seen]).max()) if seen.any() else 0.0
        print(f"{tag} seq {b} (Lq {lq}, Lk {lk}): max|diff| {err:.3e} (bar {bar:.3e}), lse {lerr:.3e}, {none} rows without keys")
        assert err <= bar, (tag, b, err, scale)
        assert lerr <= 5e-3, (tag, b, lerr)
        worst = max(worst, err / bar if bar > 0 else 0.0)
    return worst


# ---------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_batch_vs_reference(oracle_mod, D, dt, W):
    """(Without the feature the keyword is swallowed by **kwargs and the unwindowed mask runs: these cases fail there.)"""
    ins = _batch_inputs(D, dt)
    o, lse = _batch_run(D, dt, W)
    assert o.shape == ins[0].shape and o.dtype == ins[0].dtype and lse.shape == (HQ, ins[0].shape[0]) and lse.dtype == torch.float32
    worst = _check_vs_reference(oracle_mod, ins, dt, W, o, lse, _km_of_call(ins[1], ins[3], ins[4]), f"batch/d{D}/dt{dt}/W{W}")
    print(f"batch/d{D}/dt{dt}/W{W}: largest distance to the reference {worst:.3f} of its bar")
    assert torch.equal(_run(ins, **_win(W)), o)                                  # (without the LSE: the same output)
    assert not torch.equal(_run(ins, return_lse=True, **BR)[0], o)               # (the window is not ignored)


# ---------------------------------------------------------------------------------------------- 2. windows that cut no row
@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_a_window_that_cuts_no_row_gives_the_bits_of_the_call_without_it(D, dt):
    ins = _batch_inputs(D, dt)
    base = _run(ins, return_lse=True, **BR)
    lq_max, lk_max = max(p[0] for p in BATCH), max(p[1] for p in BATCH)
    for ws in ((lk_max + lq_max, 0), (2 ** 30 - 2, 0), (2 ** 30 - 2, -1)):
        _same(_run(ins, return_lse=True, **BR, window_size=ws), base, f"window_size={ws}")
    for ws in (None, (-1, -1), (-1, 0)):                                         # no window at all: the route of the call without the keyword
        _same(_run(ins, return_lse=True, **BR, window_size=ws), base, f"window_size={ws}")
    _same(_run(ins, return_lse=True, is_causal=True, window_size=(-1, 0)), _run(ins, return_lse=True, is_causal=True), "top-left, unbounded")


# ---------------------------------------------------------------------------------------------- 3. Lq = Lk on both work-list routes
@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_equal_lengths_give_the_same_bits_on_both_work_list_routes(oracle_mod, D, dt):
    ins = _inputs(tuple((n, n) for n in SQUARE), HQ, HKV, D, dt, 71 + D + dt)
    for W in (64, 200):
        a = _run(ins, return_lse=True, **_win(W))
        _same(_run(ins, return_lse=True, work_list=False, **_win(W)), a, f"Lq = Lk, W {W}, work_list=False")
    _check_vs_reference(oracle_mod, ins, dt, 200, *a, _km_of_call(ins[1], ins[3], ins[4]), f"square/d{D}/dt{dt}")


# ---------------------------------------------------------------------------------------------- 4. the ticket launch
@pytest.mark.parametrize("D", [128, 64])
def test_ticket_route_equals_the_ordinary_launch(monkeypatch, D):
    """Over the work list a large call runs as a persistent launch (the CPERS kernels).  Forced from two rounds of workgroups up, with items of
    weight 0 (blocks in front of key 0, a sequence without keys), items with both runs over the ring (head tiles, then steady tiles, with the
    pipelined diagonal or general tiles behind them) and items without head tiles among the tickets: the bits of the ordinary launch, and the
    probe confirms that the route was taken."""
    pairs = ((256, 1256), (7000, 7000), (1, 300), (3000, 3500), (6100, 6164), (511, 100), (300, 0), (700, 130))
    hq, hkv = (8, 2) if D == 128 else (16, 4)
    W = 1000
    forms = [rvw.tiles_run(rvw.loop_bounds(lq, lk, W, j)) for lq, lk in pairs for j in range((lq + 127) // 128)]
    assert any(f["head"] and f["steady"] and f["diag"] for f in forms) and any(f["head"] and f["steady"] and f["general"] for f in forms)
    assert any(not (f["head"] or f["steady"] or f["diag"] or f["general"]) for f in forms) and any(f["steady"] and not f["head"] for f in forms)
    ins = _inputs(pairs, hq, hkv, D, 1, 111 + D)
    probe = ctypes.c_int32(-1)
    monkeypatch.setattr(ops, "_PERSISTENT", False)
    with ops.launch_hooks(grid_probe=probe):
        want = _run(ins, return_lse=True, **_win(W))
    ordinary = probe.value
    monkeypatch.setattr(ops, "_PERSISTENT", True)
    with ops.launch_hooks(grid_probe=probe, force_persistent=True):
        got = _run(ins, return_lse=True, **_win(W))
    assert 0 < probe.value < ordinary
    _same(got, want, "tickets")
    none = sum(rvw.rows_without_keys(lq, lk, W) for lq, lk in pairs)
    assert int(torch.isneginf(got[1]).sum()) == hq * none and not bool(torch.isnan(got[0].float()).any())
    assert not torch.equal(got[0], _run(ins, **BR))


# ---------------------------------------------------------------------------------------------- 5. the route switches
@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_route_switches_give_the_same_bits(D, dt):
    """work_list=False (the plain kernels on the hardware's dispatch), fused_prepass=False, varlen_plan=False.  Without the plan the K mean is
    summed over other slabs, so that switch is compared with smooth_k=False, where nothing but the route differs."""
    ins = _batch_inputs(D, dt)
    for W in (100, 448):
        base = _batch_run(D, dt, W)
        for kw in (dict(work_list=False), dict(fused_prepass=False), dict(work_list=False, fused_prepass=False)):
            _same(_run(ins, return_lse=True, **_win(W), **kw), base, f"W {W}, {kw}")
        plain = _run(ins, return_lse=True, smooth_k=False, **_win(W))
        for kw in (dict(work_list=False), dict(fused_prepass=False), dict(varlen_plan=False), dict(varlen_plan=False, fused_prepass=False)):
            _same(_run(ins, return_lse=True, smooth_k=False, **_win(W), **kw), plain, f"W {W}, smooth_k=False, {kw}")


def test_padded_head_dim(oracle_mod):
    """A head dim the entry point pads (96 -> 128), on the same batch: the reference, and the plain kernels' bits."""
    ins = _inputs(BATCH, HQ, HKV, 96, 0, 67)
    o, lse = _run(ins, return_lse=True, **_win(192))
    _check_vs_reference(oracle_mod, ins, 0, 192, o, lse, _km_of_call(ins[1], ins[3], ins[4]), "batch/d96/W192")
    _same(_run(ins, return_lse=True, work_list=False, **_win(192)), (o, lse), "d96, work_list=False")


def test_more_sequences_than_the_plan_takes(oracle_mod):
    """1100 short sequences (> sage_varlen_plan_max_seqs()): no plan, no work list -- flag and window travel alone -- against the reference."""
    assert 1100 > _cabi.load().sage_varlen_plan_max_seqs()
    rng = np.random.default_rng(3)
    lq, lk = rng.integers(0, 12, size=1100), rng.integers(0, 40, size=1100)
    lq[7], lk[7] = 130, 270
    ins = _inputs(tuple(zip(lq.tolist(), lk.tolist())), 2, 1, 64, 1, 53)
    o, lse = _run(ins, return_lse=True, **_win(20))
    _check_vs_reference(oracle_mod, ins, 1, 20, o, lse, _km_of_call(ins[1], ins[3], ins[4], use_plan=False), "many")


# ---------------------------------------------------------------------------------------------- 6. what lies in front of kc0 is never read
def _operands(ins, W, dev_tensors=None):
    q, k, v, cu_q, cu_k = dev_tensors if dev_tensors is not None else [t.to(DEV) for t in ins]
    mq = max(int((ins[3][1:] - ins[3][:-1]).max()), 1)
    mk = max(int((ins[4][1:] - ins[4][:-1]).max()), 1)
    return sc._varlen_prepare(q, k, v, cu_q, cu_k, mq, mk, True, None, True, {}, v_fp8=True, bottom_right=True, window=W)


def _poison_in_front_of_kc0(st, ins, W, fill):
    """Per sequence: the INT8 key rows, the k scales and the V images of every 64-key tile in front of the first key any of its query blocks
    requests, overwritten with ``fill`` (0xFF: NaN as a k scale and as e4m3, -1 as an INT8 key; 0x5A: finite)."""
    cu_q, cu_k = ins[3].numpy(), ins[4].numpy()
    cu_ks = st.cu_ks.cpu().numpy()
    n = 0
    for b in range(len(cu_q) - 1):
        lq, lk = int(cu_q[b + 1] - cu_q[b]), int(cu_k[b + 1] - cu_k[b])
        kc0 = rvw.sequence_kc0(lq, lk, W)
        if kc0 == 0:
            continue
        k0, t0, nt = int(cu_k[b]), int(cu_ks[b]), kc0 // 64
        st.k_int8[k0:k0 + kc0].view(torch.uint8).fill_(fill)
        st.k_scale[t0:t0 + nt].view(torch.uint8).fill_(fill)
        st.v_image[t0:t0 + nt].fill_(fill)
        n += nt
    return n


@pytest.mark.parametrize("W", [1, 192])
@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_operands_in_front_of_kc0_are_never_read(D, dt, W):
    """Key rows, k scales and V images in front of each sequence's first requested key hold NaN patterns (0xFF) or 0x5A: the outputs are the
    clean run's, bit for bit.  (The attention launch's K is INT8, which has no NaN: the NaN goes where the format has one.  The pre-pass is
    the unwindowed call's and reads every key.)"""
    ins = _batch_inputs(D, dt)
    want = _batch_run(D, dt, W)
    for fill in FILLS:
        st = _operands(ins, W)
        assert _poison_in_front_of_kc0(st, ins, W, fill) >= 20
        o, lse = sc._varlen_attend_f8(st, True, True)
        torch.cuda.synchronize()
        assert torch.equal(o, want[0]), f"fill 0x{fill:02X}: o differs in {int((o != want[0]).sum())} elements"
        # (the raw LSE: log2 units, without the K-mean term the entry point adds -- compared with the clean operands' own launch)
        clean = sc._varlen_attend_f8(_operands(ins, W), True, True)
        _same((o, lse), clean, f"fill 0x{fill:02X}")


def test_nan_key_rows_in_front_of_kc0_change_nothing():
    """At the public entry, smooth_k=False (no K mean over the poisoned rows): fp16 key rows in front of each sequence's kc0 are NaN.  Their
    64-key blocks quantise to NaN scales; nothing of them is read."""
    D, dt, W = 128, 0, 100
    q, k, v, cu_q, cu_k = _batch_inputs(D, dt)
    want = _run((q, k, v, cu_q, cu_k), return_lse=True, smooth_k=False, **_win(W))
    kn = k.clone()
    for b, (lq, lk) in enumerate(BATCH):
        kn[int(cu_k[b]):int(cu_k[b]) + rvw.sequence_kc0(lq, lk, W)] = float("nan")
    assert int(torch.isnan(kn).any(dim=-1).any(dim=-1).sum()) >= 64 * 20
    _same(_run((q, kn, v, cu_q, cu_k), return_lse=True, smooth_k=False, **_win(W)), want, "NaN key rows")


@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_batch_inside_the_fence(D, dt):
    """Every buffer the package allocates between two guards and poisoned (0xFF: NaN patterns, 0x5A): no guard byte changes, the results are
    the unfenced run's -- on the work list and on the hardware's dispatch, and with the operands in front of kc0 poisoned with the fill."""
    ins = _batch_inputs(D, dt)
    W = 100
    want = _batch_run(D, dt, W)
    for fill in FILLS:
        for kw in (dict(), dict(work_list=False)):
            with Fence(fill) as f:
                got = _call(*[f.input(t) for t in ins], return_lse=True, **_win(W), **kw)
                f.check()
                assert f.package_sites() and f.owns(got[0])
                _same(got, want, f"fill 0x{fill:02X}, fenced, {kw}")
        with Fence(fill) as f:
            st = _operands(ins, W, [f.input(t) for t in ins])
            assert _poison_in_front_of_kc0(st, ins, W, fill) >= 20
            o, _ = sc._varlen_attend_f8(st, True, True)
            f.check()
            assert f.owns(o) and torch.equal(o, want[0]), f"fill 0x{fill:02X}, fenced, poisoned in front of kc0"


# ---------------------------------------------------------------------------------------------- 7. GQA 32 / 8
def test_gqa_32_8_vs_reference(oracle_mod):
    pairs = ((129, 300), (1, 200), (16, 65), (200, 70), (64, 256), (5, 0))
    ins = _inputs(pairs, 32, 8, 128, 1, 43)
    o, lse = _run(ins, return_lse=True, **_win(70))
    _check_vs_reference(oracle_mod, ins, 1, 70, o, lse, _km_of_call(ins[1], ins[3], ins[4]), "gqa32_8")
