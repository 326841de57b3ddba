"""GPU: per-sample key lengths (``kv_lens``) of the dense FP8-PV entry point.

The defining property is bit equality: sample b of a ``kv_lens`` call is the plain call on ``(q[b:b+1], k[b:b+1, :, :len_b], v[b:b+1, :, :len_b])``,
output and LSE, so almost every comparison here is ``torch.equal``.  The one tolerance is the default routes' bar against the CPU oracle
(``2e-3 max|ref| + one output ulp``, LSE within 5e-3: the form of test_gpu_parity.py::test_edge_shapes_vs_oracle).

Shapes -- the smallest that reach every loop kind of the kernel: B = 6, Hq = 4, Hkv = 2, Lk = 640 and the lengths
  640  steady tiles through all six bodies of the pipelined loop        1    a lone ragged tile
  64   one whole tile                                                   130  two whole tiles and a ragged one, no steady tile
  200  one steady tile and the tail kinds                               577  seven steady tiles and the ragged tail
with Lq = 200 for non-causal calls (a half-empty last query block) and Lq = 640 for causal ones (the diagonal crosses every sample's length
inside a query block).  The padding rows of the shared operands hold random data, so a kernel that attended to them would not pass.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util
from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, processors, quant as sq
    DEV = torch.device("cuda:0")

B, HQ, HKV, LK = 6, 4, 2, 640
LENS = (640, 1, 64, 130, 200, 577)
F16, BF16 = torch.float16, torch.bfloat16
FP8 = lambda *a, **kw: sa.sageattn_qk_int8_pv_fp8_cuda(*a, **kw)

# (D, dtype, causal, layout, smooth_k): every head dim x dtype x mask kind, the layouts and smooth_k alternating over them, and the four
# (layout, smooth_k) pairs at D = 128 in both mask kinds
CASES = [(D, dt, c, ("HND", "NHD")[(i + j + c) & 1], bool((i + c) & 1))
         for i, D in enumerate((64, 128, 96)) for j, dt in enumerate((F16, BF16)) for c in (False, True)]
CASES += [(128, F16, c, lay, sk) for c in (False, True) for lay in ("HND", "NHD") for sk in (False, True)
          if (128, F16, c, lay, sk) not in CASES]
IDS = [f"d{D}-{'f16' if dt == F16 else 'bf16'}-{'c' if c else 'nc'}-{lay}-{'sk' if sk else 'nosk'}" for D, dt, c, lay, sk in CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _lay(t, layout):
    return t if layout == "HND" else t.transpose(1, 2).contiguous()


def _cut(t, b, n, layout):
    """Sample b's first n rows as a contiguous batch of one."""
    return (t[b:b + 1, :, :n] if layout == "HND" else t[b:b + 1, :n]).contiguous()


def _hnd(t, layout):
    return t if layout == "HND" else t.transpose(1, 2)


def _qkv(D, dt, causal, layout, nb=B, seed=7):
    g = torch.Generator().manual_seed(seed + D + 2 * causal)
    lq = LK if causal else 200
    q = torch.randn(nb, HQ, lq, D, generator=g).to(dt)
    k = (torch.randn(nb, HKV, LK, D, generator=g) + torch.randn(1, HKV, 1, D, generator=g)).to(dt)
    v = torch.randn(nb, HKV, LK, D, generator=g).to(dt)
    return tuple(_lay(t.to(DEV), layout) for t in (q, k, v))


def _lens(values, dtype=torch.int32):
    return torch.tensor(list(values), dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(D, dt, causal, layout, smooth_k):
    """One ``kv_lens`` call and the plain calls on its samples' slices: computed once, shared by the tests below, never modified."""
    q, k, v = _qkv(D, dt, causal, layout)
    kw = dict(tensor_layout=layout, is_causal=causal, smooth_k=smooth_k, return_lse=True)
    o, lse = FP8(q, k, v, kv_lens=_lens(LENS), **kw)
    sliced = [FP8(q[b:b + 1], _cut(k, b, n, layout), _cut(v, b, n, layout), **kw) for b, n in enumerate(LENS)]
    torch.cuda.synchronize()
    return q, k, v, kw, o, lse, sliced


def _poisoned(t, lens, layout, byte):
    """``t`` with the rows from each sample's length on overwritten with ``byte`` (None: zeros)."""
    out = t.clone()
    raw = _hnd(out, layout).view(torch.int16)
    fill = 0 if byte is None else int(np.array([byte, byte], dtype=np.uint8).view(np.int16)[0])
    for b, n in enumerate(lens):
        raw[b, :, max(0, min(n, LK)):] = fill
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_sample_is_the_plain_call_on_its_slice(case):
    """Bit equality of o and lse, sample by sample.  (Without the feature the argument is ignored and the padding attended to.)"""
    q, k, v, kw, o, lse, sliced = _case(*case)
    assert o.shape == q.shape and lse.shape == (B, HQ, _hnd(q, case[3]).shape[2])
    for b, n in enumerate(LENS):
        ob, lb = sliced[b]
        assert torch.equal(o[b:b + 1], ob), f"sample {b} (len {n}): o differs in {int((o[b:b + 1] != ob).sum())} of {ob.numel()} elements"
        assert torch.equal(lse[b:b + 1], lb), f"sample {b} (len {n}): lse differs in {int((lse[b:b + 1] != lb).sum())} of {lb.numel()} rows"
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all())


@pytest.mark.parametrize("case", [c for c in CASES[:12]], ids=IDS[:12])
def test_samples_vs_oracle(oracle_mod, case):
    """Per sample against the CPU oracle on the sliced operands (km from the library's mean of the slice): the default routes' bar."""
    D, dt, causal, layout, smooth_k = case
    q, k, v, kw, o, lse, _ = _case(*case)
    code = 0 if dt == F16 else 1
    for b, n in enumerate(LENS):
        qb, kb, vb = (_hnd(t, layout).contiguous() for t in (q[b:b + 1], _cut(k, b, n, layout), _cut(v, b, n, layout)))
        km = None
        if smooth_k:
            kp = kb if D in (64, 128) else F.pad(kb, (0, 128 - D))
            km = util.bits(sq.channel_mean(kp))
        ref, lse_ref, _ = oracle_mod.sageattn_dense(util.bits(qb), util.bits(kb), util.bits(vb), code, is_causal=causal, pv="f8",
                                                    qk_quant_gran="per_thread", return_lse=True, km=km, smooth_k=smooth_k, fp8_scores="exact")
        got, ref = _hnd(o[b:b + 1], layout).float().cpu().numpy(), util.f32(ref, code)
        scale = float(np.abs(ref).max())
        err, lerr = float(np.abs(got - ref).max()), float(np.abs(lse[b:b + 1].cpu().numpy() - lse_ref).max())
        print(f"sample {b} len {n}: max|diff| {err:.3e} (bar {2e-3 * scale + util.out_ulp(scale, code):.3e}), lse {lerr:.3e}")
        assert np.isfinite(got).all()
        assert err <= 2e-3 * scale + util.out_ulp(scale, code), (b, n)
        assert lerr <= 5e-3, (b, n)


@pytest.mark.parametrize("case", [CASES[2], CASES[5], CASES[9]], ids=[IDS[2], IDS[5], IDS[9]])
def test_padding_is_never_read(case):
    """Padding rows of k and v as zeros, 0xFF bytes (NaN) and 0x5A bytes: the same finite bits as with the random padding of the shared
    case -- plainly, and inside the fenced, poisoned allocator, where every K row, scale slot and V tile the pre-pass leaves unwritten is
    NaN (then 0x5A) as well, no guard byte may change, and the allocations must be those of the kv_lens route."""
    D, dt, causal, layout, smooth_k = case
    q, k, v, kw, o, lse, _ = _case(*case)
    lens = _lens(LENS)
    for byte in (None, 0xFF, 0x5A):
        kp, vp = _poisoned(k, LENS, layout, byte), _poisoned(v, LENS, layout, byte)
        o2, lse2 = FP8(q, kp, vp, kv_lens=lens, **kw)
        assert torch.equal(o2, o) and torch.equal(lse2, lse), f"padding byte {byte}: the result depends on the padding"
    for fill in FILLS:
        kp, vp = _poisoned(k, LENS, layout, fill), _poisoned(v, LENS, layout, fill)
        with Fence(fill) as f:
            o3, lse3 = FP8(f.input(q), f.input(kp), f.input(vp), kv_lens=f.input(lens), **kw)
            f.check()
            assert torch.equal(o3, o) and torch.equal(lse3, lse), f"fill 0x{fill:02X}: the fenced run differs"
            funcs = {a[0] for a in f.package_allocations()}
            assert {"per_thread_int8_k_kvlens", "per_channel_fp8_kvlens"} <= funcs and ("channel_mean_kvlens" in funcs) == smooth_k, funcs
            assert not funcs & {"prepass_kv_fp8", "per_channel_fp8", "_quant", "channel_mean"}, funcs
            if D in (64, 128):
                assert f.owns(o3)
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all())


@pytest.mark.parametrize("D,dt,causal,layout", [(128, F16, False, "HND"), (64, BF16, True, "NHD")])
def test_edges(D, dt, causal, layout):
    kw = dict(tensor_layout=layout, is_causal=causal, return_lse=True)
    # empty samples: zeros and -inf, no NaN; their neighbour is the plain call
    q, k, v = _qkv(D, dt, causal, layout, nb=3)
    for byte in (None, 0xFF):
        lens = (0, LK, 0)
        o, lse = FP8(q, _poisoned(k, lens, layout, byte), _poisoned(v, lens, layout, byte), kv_lens=_lens(lens), **kw)
        o1, lse1 = FP8(q[1:2], k[1:2], v[1:2], **kw)
        for b in (0, 2):
            assert bool((o[b] == 0).all()) and bool((lse[b] == float("-inf")).all()), (b, byte)
        assert torch.equal(o[1:2], o1) and torch.equal(lse[1:2], lse1)
        assert not bool(o.isnan().any()) and not bool(lse.isnan().any())
    # lengths out of range are clamped on the device
    a = FP8(q[:2], k[:2], v[:2], kv_lens=_lens((LK + 100, -5)), **kw)
    b_ = FP8(q[:2], k[:2], v[:2], kv_lens=_lens((LK, 0)), **kw)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])
    # all lengths full: the call without kv_lens
    full = FP8(q, k, v, kv_lens=_lens((LK, LK, LK)), **kw)
    plain = FP8(q, k, v, **kw)
    assert torch.equal(full[0], plain[0]) and torch.equal(full[1], plain[1])


def test_int64_lengths_and_the_forwarding_callers():
    case = CASES[2]
    D, dt, causal, layout, smooth_k = case
    q, k, v, kw, o, lse, _ = _case(*case)
    o64, lse64 = FP8(q, k, v, kv_lens=_lens(LENS, torch.int64), **kw)
    assert torch.equal(o64, o) and torch.equal(lse64, lse)
    # sageattn forwards to the FP8 entry point with pv_accum_dtype="fp32+fp32" and smooth_k=True
    ref = FP8(q, k, v, kv_lens=_lens(LENS), tensor_layout=layout, is_causal=causal, return_lse=True, pv_accum_dtype="fp32+fp32")
    got = sa.sageattn(q, k, v, tensor_layout=layout, is_causal=causal, return_lse=True, kv_lens=_lens(LENS))
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    got = processors.sdpa(q, k, v, is_causal=causal, tensor_layout=layout, kv_lens=_lens(LENS))
    assert torch.equal(got, ref[0])
    assert not torch.equal(got, sa.sageattn(q, k, v, tensor_layout=layout, is_causal=causal))        # (the lengths are not ignored)


@pytest.mark.parametrize("causal", [False, True])
def test_graph_capture_follows_the_lengths_tensor(causal):
    """Captured once; each replay computes with what the lengths tensor holds then: no host read, no decision on the host."""
    D, dt, layout = 128, F16, "HND"
    q, k, v = _qkv(D, dt, causal, layout)
    kw = dict(tensor_layout=layout, is_causal=causal, return_lse=True)
    first, second = LENS, (3, 640, 0, 129, 448, 65)
    lens = _lens(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        FP8(q, k, v, kv_lens=lens, **kw)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o, lse = FP8(q, k, v, kv_lens=lens, **kw)
    for values in (second, first):
        lens.copy_(_lens(values))
        g.replay()
        eo, el = FP8(q, k, v, kv_lens=_lens(values), **kw)
        torch.cuda.synchronize()
        assert torch.equal(o, eo) and torch.equal(lse, el), values
