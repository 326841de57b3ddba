"""GPU: bottom-right causal alignment of the packed FP8-PV route, ``sageattn_qk_int8_pv_fp8_varlen(causal_align="bottom_right")``.

Row i of sequence b attends to key j of that sequence iff ``j <= i + Lk_b - Lq_b``.  References:
  * the exact CPU oracle with the shift restated by padding (tests/ref_varlen_br.py), every sequence at the packed route's own bar,
    ``2e-3 max|o| + one output ulp`` and LSE within 5e-3 (test_gpu_varlen_fp8.py);
  * bit identities: offsets that are multiples of 128 against the top-left packed call with that many junk rows in front of each sequence's q
    (the same 128-row Q groups, the same K mean over all packed tokens, the same per-sequence V scales); ``Lq = Lk`` throughout against the
    call without the keyword; the route switches; the ticket launch against the ordinary one; the run inside the fenced allocator.

BATCH holds the shapes at which the kernel can go wrong, one packed call (GQA 4 / 2, D 64 and 128, fp16 and bf16):
  (200, 640) offset 440: three general tiles on the diagonal behind steady ones     (128, 512) offset 384: the pipelined diagonal bodies
  (1, 300) decode     (16, 1000) speculative verification     (300, 130) offset -170: rows in front of key 0 in one block and tile with rows
  that see keys     (260, 1) a lone key     (70, 0) no keys     (0, 50) no rows     (129, 129) offset 0     (5, 64) few rows against one whole tile
(tests/test_varlen_br_host.py::test_loop_bounds_of_the_tested_batch holds the tile counts they reach.)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import util
import ref_varlen_br as rb
from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, core as sc, ops, quant as sq
    DEV = torch.device("cuda:0")

BATCH = ((200, 640), (128, 512), (1, 300), (16, 1000), (300, 130), (260, 1), (70, 0), (0, 50), (129, 129), (5, 64))
ALIGNED = ((200, 200), (130, 258), (64, 320), (300, 684), (1, 385), (129, 257), (128, 128))      # offsets 0, 128, 256, 384, 384, 128, 0
SQUARE = (1, 63, 64, 0, 65, 127, 129, 1000)
GRID = [(64, 0), (64, 1), (128, 0), (128, 1)]
IDS = [f"d{D}-{'f16' if dt == 0 else 'bf16'}" for D, dt in GRID]
HQ, HKV = 4, 2
BR = dict(is_causal=True, causal_align="bottom_right")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _tdt(dt):
    return torch.float16 if dt == 0 else torch.bfloat16


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _inputs(pairs, Hq, Hkv, D, dt, seed):
    """q [sum Lq, Hq, D], k / v [sum Lk, Hkv, D] (K with a per-channel bias) on the CPU, cu_q, cu_k: made once per case, never modified."""
    lq, lk = [p[0] for p in pairs], [p[1] for p in pairs]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(sum(lq), Hq, D, generator=g).to(_tdt(dt))
    k = (torch.randn(sum(lk), Hkv, D, generator=g) + torch.randn(1, Hkv, D, generator=g)).to(_tdt(dt))
    v = torch.randn(sum(lk), Hkv, D, generator=g).to(_tdt(dt))
    return q, k, v, _cu(lq), _cu(lk)


def _call(q, k, v, cu_q, cu_k, **kw):
    mq = max(int((cu_q[1:] - cu_q[:-1]).max()), 1)
    mk = max(int((cu_k[1:] - cu_k[:-1]).max()), 1)
    return sa.sageattn_qk_int8_pv_fp8_varlen(q, k, v, cu_q, cu_k, mq, mk, **kw)


def _run(ins, **kw):
    q, k, v, cu_q, cu_k = ins
    out = _call(q.to(DEV), k.to(DEV), v.to(DEV), cu_q.to(DEV), cu_k.to(DEV), **kw)
    torch.cuda.synchronize()
    return out


def _km_of_call(k, cu_q, cu_k, use_plan=True):
    """The K mean the call forms: over ALL packed tokens, summed over the plan's per-sequence slabs (or packed slabs without a plan)."""
    kd, cq, ck = sc._pad_head_dim(*(k.to(DEV),) * 3)[0], cu_q.to(DEV), cu_k.to(DEV)
    plan = sq.varlen_plan(cq, ck, total_q=int(cu_q[-1]), total_k=k.shape[0]) if use_plan else None
    return util.bits(sq.channel_mean_packed(kd, ck, plan))


@functools.lru_cache(maxsize=None)
def _batch_run(D, dt):
    """BATCH through the default route with the LSE: (o, lse) on the device.  Shared by the oracle, the closed-form and the fence cases."""
    return _run(_inputs(BATCH, HQ, HKV, D, dt, 7 + D + dt), return_lse=True, **BR)


def _same(a, b, what=""):
    assert torch.equal(a[0], b[0]), f"{what}: o differs in {int((a[0] != b[0]).sum())} of {a[0].numel()} elements"
    assert torch.equal(a[1], b[1]), f"{what}: lse differs in {int((a[1] != b[1]).sum())} of {a[1].numel()} rows"


def _check_vs_oracle(O, ins, dt, o, lse, km, tag):
    """Every sequence: max|diff| <= 2e-3 max|o| + one output ulp at max|o|; LSE within 5e-3; rows that see nothing exactly +0 / -inf."""
    q, k, v, cu_q, cu_k = ins
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
        assert not got[s:s + none].any() and not np.signbit(got[s:s + none]).any(), (tag, b)            # +0, not merely small
        scale = float(np.abs(ref[s:e]).max())
        err = float(np.abs(got[s:e] - ref[s:e]).max())
        seen = ~empty[:, s:e]
        lerr = float(np.abs(lgot[:, s:e][seen] - lse_ref[:, s:e][seen]).max()) if seen.any() else 0.0
        print(f"{tag} seq {b} (Lq {lq}, Lk {lk}): max|diff| {err:.3e} (bar {2e-3 * scale + util.out_ulp(scale, dt):.3e}), lse {lerr:.3e}, "
              f"{none} rows without keys")
        assert err <= 2e-3 * scale + util.out_ulp(scale, dt), (tag, b, err, scale)
        assert lerr <= 5e-3, (tag, b, lerr)


# ---------------------------------------------------------------------------------------------- 1. the exact CPU oracle
@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_batch_vs_oracle(oracle_mod, D, dt):
    """(Without the feature the keyword is swallowed by **kwargs and the top-left mask runs: this case fails there.)"""
    ins = _inputs(BATCH, HQ, HKV, D, dt, 7 + D + dt)
    o, lse = _batch_run(D, dt)
    assert o.shape == ins[0].shape and o.dtype == ins[0].dtype and lse.shape == (HQ, ins[0].shape[0]) and lse.dtype == torch.float32
    _check_vs_oracle(oracle_mod, ins, dt, o, lse, _km_of_call(ins[1], ins[3], ins[4]), f"batch/d{D}/dt{dt}")
    assert torch.equal(_run(ins, **BR), o)                                   # (without the LSE: the same output)
    assert not torch.equal(_run(ins, is_causal=True), o)                     # (the alignment is not ignored)


@pytest.mark.parametrize("smooth_k", [True, False])
def test_batch_vs_oracle_without_smoothing_and_padded_head_dim(oracle_mod, smooth_k):
    """smooth_k=False, and a head dim the entry point pads (96 -> 128), on the same batch."""
    D, dt = (96, 0) if smooth_k else (128, 1)
    ins = _inputs(BATCH, HQ, HKV, D, dt, 17 + D)
    o, lse = _run(ins, return_lse=True, smooth_k=smooth_k, **BR)
    km = _km_of_call(ins[1], ins[3], ins[4]) if smooth_k else None
    _check_vs_oracle(oracle_mod, ins, dt, o, lse, km, f"batch/d{D}/{'sk' if smooth_k else 'nosk'}")


# ---------------------------------------------------------------------------------------------- 2. offsets that line the blocks up
@pytest.mark.parametrize("smooth_k", [False, True], ids=["nosk", "sk"])
@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_aligned_offsets_are_the_padded_top_left_call(D, dt, smooth_k):
    """Offsets in {0, 128, 256, 384}: the bits of the existing top-left packed call with that many junk rows in front of each sequence's q.
    o on the real rows; the lse with smooth_k=False (with smoothing the entry point adds q . km, a torch matmul whose last bit depends on
    the GEMM's shape)."""
    q, k, v, cu_q, cu_k = _inputs(ALIGNED, HQ, HKV, D, dt, 23 + D + dt)
    g = torch.Generator().manual_seed(5)
    parts, rows, lq_pad = [], [], []
    at = 0
    for b, (lq, lk) in enumerate(ALIGNED):
        s = lk - lq
        assert s in (0, 128, 256, 384)
        parts += [(3.0 * torch.randn(s, HQ, D, generator=g)).to(q.dtype), q[int(cu_q[b]):int(cu_q[b + 1])]]
        rows += list(range(at + s, at + s + lq))
        at += s + lq
        lq_pad.append(s + lq)
    qp = torch.cat(parts)
    got = _run((q, k, v, cu_q, cu_k), return_lse=True, smooth_k=smooth_k, **BR)
    pad = _run((qp, k, v, _cu(lq_pad), cu_k), return_lse=True, smooth_k=smooth_k, is_causal=True)
    rows = torch.tensor(rows, device=DEV)
    assert torch.equal(got[0], pad[0][rows]), f"o differs in {int((got[0] != pad[0][rows]).sum())} elements"
    if not smooth_k:
        assert torch.equal(got[1], pad[1][:, rows]), f"lse differs in {int((got[1] != pad[1][:, rows]).sum())} rows"
    assert bool(torch.isfinite(got[0].float()).all()) and bool(torch.isfinite(got[1]).all())


# ---------------------------------------------------------------------------------------------- 3. Lq = Lk: the call without the keyword
@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_equal_lengths_give_the_bits_of_the_top_left_call(D, dt):
    ins = _inputs(tuple((n, n) for n in SQUARE), HQ, HKV, D, dt, 31 + D + dt)
    for kw in (dict(), dict(work_list=False)):
        _same(_run(ins, return_lse=True, **BR, **kw), _run(ins, return_lse=True, is_causal=True, **kw), f"Lq = Lk {kw}")
    _same(_run(ins, return_lse=True, is_causal=True, causal_align="top_left"), _run(ins, return_lse=True, is_causal=True), "top_left")


# ---------------------------------------------------------------------------------------------- 4. rows without keys
@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_rows_without_keys_are_zero_and_minus_infinity(D, dt):
    o, lse = _batch_run(D, dt)
    assert not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(lse).any()) and not bool((lse == float("inf")).any())
    of, at, total = o.float(), 0, 0
    for lq, lk in BATCH:
        none = rb.rows_without_keys(lq, lk)
        total += none
        assert bool(torch.isneginf(lse[:, at:at + none]).all()) and bool(torch.isfinite(lse[:, at + none:at + lq]).all()), (lq, lk)
        assert not bool(of[at:at + none].any()) and not bool(torch.signbit(of[at:at + none]).any()), (lq, lk)
        at += lq
    assert total == 170 + 259 + 70 and int(torch.isneginf(lse).sum()) == HQ * total


# ---------------------------------------------------------------------------------------------- 5. the route switches
@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_route_switches_give_the_same_bits(D, dt):
    """work_list=False (the plain kernels on the hardware's dispatch), fused_prepass=False, varlen_plan=False.  Without the plan the K mean is
    summed over other slabs (equal up to an input-dtype rounding, as sageattn_varlen's docstring says), so that switch is compared with
    smooth_k=False, where nothing but the route differs; the other two with and without smoothing."""
    ins = _inputs(BATCH, HQ, HKV, D, dt, 7 + D + dt)
    base = _batch_run(D, dt)
    for kw in (dict(work_list=False), dict(fused_prepass=False), dict(fused_prepass=True), dict(work_list=False, fused_prepass=False)):
        _same(_run(ins, return_lse=True, **BR, **kw), base, str(kw))
    plain = _run(ins, return_lse=True, smooth_k=False, **BR)
    for kw in (dict(work_list=False), dict(fused_prepass=False), dict(varlen_plan=False), dict(varlen_plan=False, fused_prepass=False)):
        _same(_run(ins, return_lse=True, smooth_k=False, **BR, **kw), plain, f"smooth_k=False, {kw}")


def test_more_sequences_than_the_plan_takes(oracle_mod):
    """1100 short sequences (> sage_varlen_plan_max_seqs()): no plan, no work list -- the flag travels alone -- against the oracle."""
    assert 1100 > _cabi.load().sage_varlen_plan_max_seqs()
    rng = np.random.default_rng(3)
    lq, lk = rng.integers(0, 12, size=1100), rng.integers(0, 40, size=1100)
    lq[7], lk[7] = 130, 70
    ins = _inputs(tuple(zip(lq.tolist(), lk.tolist())), 2, 1, 64, 1, 51)
    o, lse = _run(ins, return_lse=True, **BR)
    _check_vs_oracle(oracle_mod, ins, 1, o, lse, _km_of_call(ins[1], ins[3], ins[4], use_plan=False), "many")


@pytest.mark.parametrize("D", [128, 64])
def test_ticket_route_equals_the_ordinary_launch(monkeypatch, D):
    """Over the work list a large call runs as a persistent launch (the CPERS kernels).  Forced from two rounds of workgroups up, with items of
    weight 0 (blocks in front of key 0, a sequence without keys) among the tickets: the bits of the ordinary launch, and the probe confirms
    that the route was taken."""
    pairs = ((256, 1256), (7000, 7000), (1, 300), (3000, 3500), (6100, 6164), (511, 100), (300, 0), (700, 130))
    hq, hkv = (8, 2) if D == 128 else (16, 4)              # (D = 64 holds three workgroups per CU: two rounds of them are more items)
    ins = _inputs(pairs, hq, hkv, D, 1, 111 + D)
    probe = ctypes.c_int32(-1)
    monkeypatch.setattr(ops, "_PERSISTENT", False)
    with ops.launch_hooks(grid_probe=probe):
        want = _run(ins, return_lse=True, **BR)
    ordinary = probe.value
    monkeypatch.setattr(ops, "_PERSISTENT", True)
    with ops.launch_hooks(grid_probe=probe, force_persistent=True):
        got = _run(ins, return_lse=True, **BR)
    assert 0 < probe.value < ordinary
    _same(got, want, "tickets")
    none = sum(rb.rows_without_keys(lq, lk) for lq, lk in pairs)
    assert int(torch.isneginf(got[1]).sum()) == hq * none and not bool(torch.isnan(got[0].float()).any())


# ---------------------------------------------------------------------------------------------- 6. the device-built plan
def test_the_device_built_plan_equals_the_host_view():
    """sage_varlen_plan(is_causal=2) against sage_debug_varlen_items: the same functions of sage_work_order.h on either side."""
    lib = _cabi.load()
    g = torch.Generator().manual_seed(6)
    sets = [(torch.tensor([p[0] for p in BATCH]), torch.tensor([p[1] for p in BATCH]))]
    for nseq in (1, 2, 7, 64, 333, 1024):
        hi = 5000 if nseq < 300 else 700
        lq, lk = torch.randint(0, hi, (nseq,), generator=g), torch.randint(0, hi, (nseq,), generator=g)
        lk[::3] = lq[::3] // 2                       # more rows than keys: blocks of weight 0
        lk[1::7] = 0
        sets.append((lq, lk))
    for lq, lk in sets:
        nseq = lq.numel()
        cu_q = torch.nn.functional.pad(lq.cumsum(0), (1, 0)).to(torch.int32).to(DEV)
        cu_k = torch.nn.functional.pad(lk.cumsum(0), (1, 0)).to(torch.int32).to(DEV)
        plan = sq.varlen_plan(cu_q, cu_k, total_q=int(lq.sum()), total_k=int(lk.sum()), is_causal=2, Hq=12, Hkv=4, head_dim=128, pv_fp8=True)
        nitems = int(((lq + 127) // 128).sum())
        hdr = plan.hdr.cpu().numpy()
        assert hdr[0] == nitems <= plan.items_bound
        lqa, lka = lq.numpy().astype(np.int32), lk.numpy().astype(np.int32)
        items, hh = np.zeros((max(nitems, 1), 2), np.int32), np.zeros(8, np.int32)
        grid = lib.sage_debug_varlen_items(lqa.ctypes.data_as(ctypes.c_void_p), lka.ctypes.data_as(ctypes.c_void_p), nseq, 2, 12, 4, 128, 1,
                                           items.ctypes.data_as(ctypes.c_void_p), max(nitems, 1), hh.ctypes.data_as(ctypes.c_void_p))
        assert grid >= 0 and (hh[:4] == hdr[:4]).all()
        dev_items = plan.items.cpu().numpy()[:nitems]
        assert (dev_items == items[:nitems]).all(), nseq
        ws = [rb.item_weight(int(lqa[s]), int(lka[s]), int(j)) for s, j in dev_items]
        assert ws == sorted(ws, reverse=True)


# ---------------------------------------------------------------------------------------------- 7. inside the fenced allocator
@pytest.mark.parametrize("D,dt", GRID, ids=IDS)
def test_batch_inside_the_fence(D, dt):
    """Every buffer the package allocates between two guards and poisoned (0xFF: NaN patterns, 0x5A): no guard byte changes, the results
    are the unfenced run's, the output lives in a fenced arena -- on the work list and on the hardware's dispatch."""
    ins = _inputs(BATCH, HQ, HKV, D, dt, 7 + D + dt)
    want = _batch_run(D, dt)
    for fill in FILLS:
        for kw in (dict(), dict(work_list=False)):
            with Fence(fill) as f:
                got = _call(*[f.input(t) for t in ins], return_lse=True, **BR, **kw)
                f.check()
                assert f.package_sites() and f.owns(got[0])
                _same(got, want, f"fill 0x{fill:02X}, fenced, {kw}")


# ---------------------------------------------------------------------------------------------- 8. GQA 32 / 8
@pytest.mark.parametrize("dt", [0, 1])
def test_gqa_32_8_vs_oracle(oracle_mod, dt):
    pairs = ((129, 300), (1, 200), (16, 65), (200, 70), (64, 256), (5, 0))
    ins = _inputs(pairs, 32, 8, 128, dt, 41 + dt)
    o, lse = _run(ins, return_lse=True, **BR)
    _check_vs_oracle(oracle_mod, ins, dt, o, lse, _km_of_call(ins[1], ins[3], ins[4]), f"gqa32_8/dt{dt}")
