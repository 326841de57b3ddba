"""GPU: the sliding window of the dense FP8-PV entry point (``window_size=``).

Row i of sample b attends to key j iff ``s_b + r + i - W < j <= s_b + r + i`` and ``0 <= j < len_b``.  References:
  * ``tests/ref_window.py`` -- the kernel arithmetic with a visibility predicate, pinned to the C oracle on the CPU (test_window_host.py) -- on
    the quantised operands the oracle's ``sageattn_dense`` returns for the sample's valid keys.  The bar is the default routes' own with one
    more output ulp, the restatement's pinned distance to the oracle: ``2e-3 max|ref| + 2 output ulps``, LSE within 5e-3; rows whose window
    holds no key are exactly ``+0`` / ``-inf`` and are the predicate's rows;
  * a window that cuts no row is, bit for bit, the call without the keyword;
  * operands in front of a sample's first visible tile and behind its length, overwritten with NaN patterns and 0x5A bytes, change no bit.

Shapes are test_gpu_q_start.py's: B = 6, Hq = 4, Hkv = 2, Lk = 640, Lq = 200 (a half-empty second query block), D in {64, 128, 96}; the
padding rows of k / v hold random data.  The cases -- (len, offset, window), two batches of six -- are ``ref_window.WINDOW_CASES``.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util
import ref_window as rw
from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention as mirror
    import sageattention_amd as sa
    from sageattention_amd import _cabi, core, processors, quant as sq
    DEV = torch.device("cuda:0")

B, HQ, HKV, LK, LQ = 6, 4, 2, rw.LK, rw.LQ
LENS = (640, 577, 200, 130, 64, 1)
ALIGNED = (0, 128, 256, 384)
F16, BF16 = torch.float16, torch.bfloat16
FP8 = lambda *a, **kw: sa.sageattn_qk_int8_pv_fp8_cuda(*a, **kw)

# (D, dtype, layout, smooth_k): test_gpu_q_start.py's grid
CASES = [(D, dt, ("HND", "NHD")[(i + j) & 1], bool(i & 1) != bool(j)) for i, D in enumerate((64, 128, 96)) for j, dt in enumerate((F16, BF16))]
CASES += [(128, F16, lay, sk) for lay in ("HND", "NHD") for sk in (False, True) if (128, F16, lay, sk) not in CASES]
IDS = [f"d{D}-{'f16' if dt == F16 else 'bf16'}-{lay}-{'sk' if sk else 'nosk'}" for D, dt, lay, sk in CASES]


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
def _qkv(D, dt, layout, lq=LQ, seed=11):
    """q [B, HQ, lq, D], k / v [B, HKV, LK, D] in ``layout``: made once per case, never modified."""
    g = torch.Generator().manual_seed(seed + D + lq)
    q = torch.randn(B, HQ, lq, D, generator=g).to(dt)
    k = (torch.randn(B, HKV, LK, D, generator=g) + torch.randn(1, HKV, 1, D, generator=g)).to(dt)
    v = torch.randn(B, HKV, LK, D, generator=g).to(dt)
    return tuple(_lay(t.to(DEV), layout) for t in (q, k, v))


def _ints(values, dtype=torch.int32):
    return torch.tensor(list(values), dtype=dtype, device=DEV)


def _same(a, b, what=""):
    assert torch.equal(a[0], b[0]), f"{what}: o differs in {int((a[0] != b[0]).sum())} of {a[0].numel()} elements"
    assert torch.equal(a[1], b[1]), f"{what}: lse differs in {int((a[1] != b[1]).sum())} of {a[1].numel()} rows"


# ---------------------------------------------------------------------------------------------- 1. against the predicate restatement
def _ref_sample(oracle, qb, kb, vb, code, D, smooth_k, keep):
    """Reference o (float32 [HQ, lq, D]) and lse (natural log, as the entry point returns it) of one sample under the predicate ``keep``
    [lq, n]; qb / kb / vb: HND, on the device, kb / vb cut to the sample's n valid keys."""
    lq, n = qb.shape[2], kb.shape[2]
    if n == 0:
        return np.zeros((HQ, lq, D), np.float32), np.full((HQ, lq), -np.inf, np.float32)
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
        kmf = np.repeat(oracle.to_f32(aux["km"], code), HQ // HKV, axis=1)
        corr = oracle.to_f32(oracle.convert(np.einsum("bhld,bhd->bhl", qf, kmf), kind), code)
        lse = lse + corr[0] * np.float32(1.0 / (D ** 0.5))
    return o.float().numpy()[..., :D], lse


def _check(oracle, case, q, k, v, lens, starts, W, r, o, lse):
    D, dt, layout, smooth_k = case
    code = 0 if dt == F16 else 1
    lq = _hnd(q, layout).shape[2]
    for b, (n, s) in enumerate(zip(lens, starts)):
        n_c = max(0, min(n, LK))
        qb, kb, vb = (_hnd(t, layout).contiguous() for t in (q[b:b + 1], _cut(k, b, n_c, layout), _cut(v, b, n_c, layout)))
        keep = rw.visible(lq, n_c, s, W, r, n_c)
        ref, lse_ref = _ref_sample(oracle, qb, kb, vb, code, D, smooth_k, keep)
        got, lgot = _hnd(o[b:b + 1], layout)[0].float().cpu().numpy(), lse[b].cpu().numpy()
        empty = np.broadcast_to(~keep.any(dim=1).numpy(), (HQ, lq))
        if r == 0 and W > 0:
            assert int(empty[0].sum()) == rw.rows_without_keys(lq, s, W, n_c), (b, n, s, W)
        assert np.array_equal(np.isneginf(lse_ref), empty), (b, n, s, W)
        scale = float(np.abs(ref).max())
        bar = 2e-3 * scale + 2 * util.out_ulp(scale, code)
        err = float(np.abs(got - ref).max())
        lerr = float(np.abs(lgot[~empty] - lse_ref[~empty]).max()) if (~empty).any() else 0.0
        print(f"sample {b} len {n} offset {s} window {W} shift {r}: max|diff| {err:.3e} (bar {bar:.3e}), lse {lerr:.3e}, {int(empty[0].sum())} empty rows")
        assert np.isfinite(got).all() and not np.isnan(lgot).any(), (b, n, s, W)
        assert np.array_equal(np.isneginf(lgot), empty), (b, n, s, W)                          # the rows without keys are the predicate's
        assert not got[empty].any() and not np.signbit(got[empty]).any(), (b, n, s, W)        # +0, not merely small
        assert err <= bar, (b, n, s, W, err, bar)
        assert lerr <= 5e-3, (b, n, s, W, lerr)


@pytest.mark.parametrize("case", CASES[:6], ids=IDS[:6])
def test_windows_vs_restatement(oracle_mod, case):
    """Each sample of a batch has a window of its own in the table, the keyword one per call: every case is its own call on the whole batch
    (kv_lens / q_start of the case in its slot, the other slots plain), and its slot is checked."""
    D, dt, layout, smooth_k = case
    q, k, v = _qkv(D, dt, layout)
    kw = dict(tensor_layout=layout, is_causal=True, smooth_k=smooth_k, return_lse=True)
    for batch in (rw.WINDOW_CASES[:B], rw.WINDOW_CASES[B:]):
        lens, starts = [c[0] for c in batch], [c[1] for c in batch]
        for b, (n, s, W) in enumerate(batch):
            o, lse = FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints(starts), window_size=(W - 1, 0), **kw)
            assert o.shape == q.shape and lse.shape == (B, HQ, LQ)
            _check(oracle_mod, case, q[b:b + 1], k[b:b + 1], v[b:b + 1], [n], [s], W, 0, o[b:b + 1], lse[b:b + 1])


def test_non_causal_windows(oracle_mod):
    """window_size with is_causal=False: the causal kernels with the diagonal moved right -- (100, 30), (-1, 30) against the restatement on
    every sample of a batch, with offsets and lengths; (63, 0) equals its causal spelling bit for bit."""
    case = CASES[1]
    D, dt, layout, smooth_k = case
    q, k, v = _qkv(D, dt, layout)
    kw = dict(tensor_layout=layout, smooth_k=smooth_k, return_lse=True)
    lens, starts = (640, 577, 200, 130, 64, 0), (440, 377, 0, -70, 100, 5)
    for ws, W, r in (((100, 30), 131, 30), ((-1, 30), 0, 30)):
        o, lse = FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints(starts), window_size=ws, is_causal=False, **kw)
        _check(oracle_mod, case, q, k, v, lens, starts, W, r, o, lse)
        o0, lse0 = FP8(q, k, v, window_size=ws, is_causal=False, **kw)                       # no lengths, no offsets: rows at key 0 ...
        _same((o0, lse0), FP8(q, k, v, kv_lens=_ints([LK] * B), q_start=0, window_size=ws, is_causal=False, **kw), f"{ws} without kv_lens / q_start")
        _check(oracle_mod, case, q[:1], k[:1], v[:1], [LK], [0], W, r, o0[:1], lse0[:1])
    a = FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints(starts), window_size=(63, 0), is_causal=False, **kw)
    _same(a, FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints(starts), window_size=(63, 0), is_causal=True, **kw), "(63, 0) non-causal")
    _same(a, FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints(starts), window_size=(63, -1), is_causal=True, **kw), "(63, -1) causal")
    assert not torch.equal(a[0], FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints(starts), is_causal=True, **kw)[0])      # (the window is not ignored)
    # sageattn forwards to the FP8 entry point with pv_accum_dtype="fp32+fp32" and smooth_k=True; processors.sdpa to sageattn
    ref = FP8(q, k, v, kv_lens=_ints(lens), tensor_layout=layout, is_causal=True, return_lse=True, pv_accum_dtype="fp32+fp32", window_size=(63, 0))
    _same(sa.sageattn(q, k, v, tensor_layout=layout, is_causal=True, return_lse=True, kv_lens=_ints(lens), window_size=(63, 0)), ref, "sageattn")
    _same(mirror.sageattn(q, k, v, tensor_layout=layout, is_causal=True, return_lse=True, kv_lens=_ints(lens), window_size=(63, 0)), ref, "mirror")
    assert torch.equal(processors.sdpa(q, k, v, is_causal=True, tensor_layout=layout, kv_lens=_ints(lens), window_size=(63, 0)), ref[0])


@pytest.mark.parametrize("lq", [1, 16])
def test_decode_shapes_vs_restatement(oracle_mod, lq):
    """Lq = 1 and 16 new rows at the end of each sample's keys, the last 100 keys visible."""
    case = CASES[2]
    D, dt, layout, smooth_k = case
    q, k, v = _qkv(D, dt, layout, lq=lq)
    kw = dict(tensor_layout=layout, is_causal=True, smooth_k=smooth_k, return_lse=True)
    o, lse = FP8(q, k, v, kv_lens=_ints(LENS), causal_align="bottom_right", window_size=(99, 0), **kw)
    _check(oracle_mod, case, q, k, v, LENS, [n - lq for n in LENS], 100, 0, o, lse)


# ---------------------------------------------------------------------------------------------- 2. a window that cuts no row
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_window_that_cuts_no_row_is_the_call_without_it(case):
    D, dt, layout, smooth_k = case
    q, k, v = _qkv(D, dt, layout)
    kw = dict(tensor_layout=layout, is_causal=True, smooth_k=smooth_k, return_lse=True)
    for s in ALIGNED:
        plain = FP8(q, k, v, kv_lens=_ints(LENS), q_start=_ints([s] * B), **kw)
        for left in (LK + LQ, 2 ** 30 - 1):
            _same(FP8(q, k, v, kv_lens=_ints(LENS), q_start=_ints([s] * B), window_size=(left, 0), **kw), plain, f"offset {s}, left {left}")
    plain = FP8(q, k, v, **kw)
    for left in (LK + LQ, 2 ** 30 - 1):
        _same(FP8(q, k, v, window_size=(left, 0), **kw), plain, f"no lengths, no offsets, left {left}")


# ---------------------------------------------------------------------------------------------- 3. what lies outside the window is never read
def _prepassed(q, k, v, layout, smooth_k, lens):
    D = q.shape[-1]
    qp, kp, vp, _ = core._pad_head_dim(q, k, v)
    _, _, k8, ks, vimg, vs, _ = core._prepass_kv(qp, kp, vp, layout, "per_thread", 64, smooth_k, False, False, False, kv_lens=lens)
    return core._aligned(qp, 8), k8, ks, vimg, vs, core._sm_log2(D ** -0.5)


def _poison(k8, ks, vimg, layout, lens, starts, W, byte):
    """Copies of the pre-passed operands with everything a windowed work item may not read overwritten with ``byte``: per sample the INT8 K
    rows, k scales and V-image tiles in front of the tile of its first visible key, (max(0, s - W + 1)) & ~63, and everything from its length
    on (the tile that holds the last valid key keeps its zero-padded V image and its scales)."""
    k8, ks, vimg = k8.clone(), ks.clone(), vimg.clone()
    kr = _hnd(k8, layout).view(torch.uint8)
    sr, vr = ks.view(torch.uint8).view(B, HKV, -1, 16), vimg.view(torch.uint8)          # (four float scales per 64-key tile)
    for b, (n, s) in enumerate(zip(lens, starts)):
        n = max(0, min(n, LK))
        first = min(max(0, s - W + 1) & ~63, LK)
        kr[b, :, :first] = byte
        kr[b, :, n:] = byte
        sr[b, :, :first // 64] = byte
        sr[b, :, (n + 63) // 64:] = byte
        vr[b, :, :first // 64] = byte
        vr[b, :, (n + 63) // 64:] = byte
    return k8, ks, vimg


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5]], ids=[IDS[0], IDS[3], IDS[5]])
def test_operands_outside_the_window_are_never_read(case):
    """At the attention-kernel level (core._attn_fused_q on pre-passed operands: the pre-pass statistics legitimately cover every valid key),
    plainly and once inside the fenced, poisoned allocator."""
    D, dt, layout, smooth_k = case
    q, k, v = _qkv(D, dt, layout)
    W = 100
    for batch in (rw.WINDOW_CASES[:B], rw.WINDOW_CASES[B:]):
        lens, starts = [c[0] for c in batch], [c[1] for c in batch]
        qa, k8, ks, vimg, vs, sm = _prepassed(q, k, v, layout, smooth_k, _ints(lens))
        run = lambda qa, k8, ks, vimg, vs, nl, st: core._attn_fused_q(qa, k8, vimg, vs, ks, layout, True, sm, True, kv_lens=nl, q_start=st, window=W)
        ref = run(qa, k8, ks, vimg, vs, _ints(lens), _ints(starts))
        assert not bool(torch.isnan(ref[0].float()).any()) and not bool(torch.isnan(ref[1]).any())
        for fill in FILLS:
            k8p, ksp, vimgp = _poison(k8, ks, vimg, layout, lens, starts, W, fill)
            _same(run(qa, k8p, ksp, vimgp, vs, _ints(lens), _ints(starts)), ref, f"fill 0x{fill:02X}")
        with Fence(FILLS[0]) as f:
            got = run(f.input(qa), f.input(k8p), f.input(ksp), f.input(vimgp), f.input(vs), f.input(_ints(lens)), f.input(_ints(starts)))
            f.check()
            _same(got, ref, "fenced")
            assert f.owns(got[0])


# ---------------------------------------------------------------------------------------------- 4. graph capture
def test_graph_capture_follows_lengths_and_offsets():
    """Captured once with its window (a constant of the graph); each replay computes with what kv_lens and q_start hold then."""
    D, dt, layout = 128, F16, "HND"
    q, k, v = _qkv(D, dt, layout)
    kw = dict(tensor_layout=layout, is_causal=True, return_lse=True, window_size=(99, 0))
    first = (LENS, tuple(n - LQ for n in LENS))
    second = ((3, 640, 0, 129, 448, 640), (0, 384, 7, -100, 300, 700))
    lens, starts = _ints(first[0]), _ints(first[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        FP8(q, k, v, kv_lens=lens, q_start=starts, **kw)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o, lse = FP8(q, k, v, kv_lens=lens, q_start=starts, **kw)
    for n_values, s_values in (second, first):
        lens.copy_(_ints(n_values))
        starts.copy_(_ints(s_values))
        g.replay()
        eager = FP8(q, k, v, kv_lens=_ints(n_values), q_start=_ints(s_values), **kw)
        torch.cuda.synchronize()
        _same((o, lse), eager, f"replay with {n_values} / {s_values}")
