"""GPU: ``sageattention_amd.hd256.sageattn_hd256`` (FP8-PV attention at head_dim 129 .. 256) against the CPU restatement of the reference's
FP8 route (tests/ref_fp8_torch.sageattn_fp8_cuda, whose code is written over D and runs at 256 unchanged) and against FP64 softmax attention.

Bar (the project's for every default route): |o - restatement| <= 2e-3 max|o| + one output ulp at max|o|; |lse - restatement's| <= 5e-3
(tests/test_gpu_parity.py).  Anchor: the kernel's error against FP64 softmax(q k^T sm_scale) v may exceed the restatement's own by no more than
that bar.  Each case is the smallest shape that reaches one mechanism of the kernel (a two-slot K / V ring over 64-key tiles, four waves of 32
rows, query blocks of 128)."""
import math

import pytest
import torch

import util  # noqa: F401  (sys.path)
import ref_fp8_torch as ref

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
# (Lq, Lk, causal, D, (Hq, Hkv), layout, dtype, smooth_k, sm_scale)
CASES = [
    (1, 1, False, 256, (2, 2), "HND", F16, True, None),            # minimal call
    (1, 1, True, 256, (2, 2), "NHD", BF16, True, None),
    (33, 65, False, 256, (2, 2), "HND", F16, True, None),          # partial wave, ragged second tile
    (33, 65, True, 192, (4, 2), "NHD", BF16, True, None),
    (128, 64, False, 256, (4, 2), "NHD", F16, False, None),        # exactly one tile
    (128, 64, True, 136, (2, 2), "HND", BF16, True, 0.11),
    (129, 192, False, 192, (2, 2), "HND", BF16, True, None),       # second query block, the ring wraps
    (129, 192, True, 256, (4, 2), "HND", F16, True, None),
    (257, 449, False, 256, (4, 2), "HND", BF16, True, None),       # steady state, prologue and last tile of the ring, ragged tail
    (257, 449, True, 256, (2, 2), "NHD", F16, True, 0.05),
    (257, 449, False, 136, (2, 2), "NHD", F16, False, None),
    (200, 72, True, 256, (2, 2), "HND", F16, True, None),          # rows past the last key
    (200, 72, True, 192, (4, 2), "NHD", BF16, False, None),
    (72, 200, True, 256, (4, 2), "HND", BF16, True, None),         # top-left with more keys than rows
    (72, 200, True, 136, (2, 2), "NHD", F16, True, None),
    (72, 200, False, 256, (2, 2), "HND", F16, False, 0.03),
    (33, 63, False, 256, (2, 2), "NHD", BF16, True, None),         # the last key on either side of the first and the second tile boundary
    (33, 64, False, 256, (4, 2), "HND", F16, True, None),
    (33, 65, False, 192, (2, 2), "NHD", F16, False, None),
    (33, 127, False, 256, (2, 2), "HND", BF16, True, None),
    (33, 128, False, 256, (4, 2), "NHD", F16, True, None),
    (33, 129, False, 256, (2, 2), "HND", BF16, False, None),
    (33, 129, True, 256, (2, 2), "NHD", F16, True, None),
    (127, 192, False, 256, (2, 2), "HND", F16, True, None),        # the last row on either side of the first and the second block boundary
    (127, 192, True, 256, (4, 2), "NHD", BF16, True, None),
    (128, 192, False, 256, (4, 2), "NHD", BF16, True, None),
    (128, 192, True, 256, (2, 2), "HND", F16, True, None),
    (255, 192, False, 192, (2, 2), "NHD", F16, True, None),
    (255, 192, True, 256, (2, 2), "HND", BF16, True, None),
    (256, 192, False, 256, (2, 2), "HND", BF16, False, None),
    (256, 192, True, 256, (4, 2), "NHD", F16, True, None),
    (129, 65, True, 256, (8, 1), "HND", F16, True, None),          # GQA groups of 8 and 4 at the smallest shape with two query blocks
    (129, 65, False, 256, (8, 2), "NHD", BF16, True, None),
]


def _fp64(q, k, v, causal, sm_scale):
    """softmax(q k^T sm_scale) v and its natural-log LSE in FP64, HND, GQA by repetition."""
    g = q.shape[1] // k.shape[1]
    qd, kd, vd = q.double(), k.double().repeat_interleave(g, dim=1), v.double().repeat_interleave(g, dim=1)
    s = qd @ kd.transpose(-1, -2) * sm_scale
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(1), -math.inf)
    return torch.softmax(s, dim=-1) @ vd, torch.logsumexp(s, dim=-1)


def _run(q, k, v, causal, layout, smooth_k, sm_scale):
    """(kernel o, kernel lse, restatement o, restatement lse, FP64 o) -- all HND, FP64, at the original head_dim."""
    from sageattention_amd.hd256 import sageattn_hd256
    D = q.shape[-1]
    dev = torch.device("cuda:0")
    lay = (lambda t: t.transpose(1, 2).contiguous()) if layout == "NHD" else (lambda t: t)
    o, lse = sageattn_hd256(lay(q).to(dev), lay(k).to(dev), lay(v).to(dev), tensor_layout=layout, is_causal=causal, sm_scale=sm_scale,
                            smooth_k=smooth_k, return_lse=True)
    torch.cuda.synchronize()
    assert o.dtype == q.dtype and o.shape == lay(q).shape and lse.shape == q.shape[:3] and lse.dtype == torch.float32
    o = (o.transpose(1, 2) if layout == "NHD" else o).cpu().double()
    sm = D ** -0.5 if sm_scale is None else sm_scale
    pad = lambda t: torch.nn.functional.pad(t, (0, 256 - D))
    ro, rlse, aux = ref.sageattn_fp8_cuda(pad(q), pad(k), pad(v), is_causal=causal, qk_quant_gran="per_thread", smooth_k=smooth_k, sm_scale=sm)
    rlse = rlse.double() / ref.LOG2E
    if smooth_k:     # the LSE correction of core._finish: + q . km sm_scale
        rlse = rlse + (pad(q).double() * aux["km"].double().repeat_interleave(q.shape[1] // k.shape[1], dim=1)[:, :, None, :]).sum(-1) * sm
    return o, lse.cpu().double(), ro[..., :D].double(), rlse, _fp64(q, k, v, causal, sm)


def _hold(o, lse, ro, rlse, truth, dtype):
    t_o, t_lse = truth
    scale = ro.abs().max().item()
    bar = 2e-3 * scale + (2.0 ** -10 if dtype == F16 else 2.0 ** -7) * scale
    err, err_k, err_r = (o - ro).abs().max().item(), (o - t_o).abs().max().item(), (ro - t_o).abs().max().item()
    print(f"max|o| {scale:.3e} bar {bar:.3e} | kernel-restatement {err:.3e} | kernel-fp64 {err_k:.3e} restatement-fp64 {err_r:.3e} | "
          f"lse {(lse - rlse).abs().max().item():.3e} (restatement-fp64 {(rlse - t_lse).abs().max().item():.3e})")
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    assert err <= bar
    assert err_k <= err_r + bar
    assert (lse - rlse).abs().max().item() <= 5e-3


@pytest.mark.parametrize("Lq,Lk,causal,D,heads,layout,dtype,smooth_k,sm_scale", CASES)
def test_hd256_matches_the_restatement_and_fp64(Lq, Lk, causal, D, heads, layout, dtype, smooth_k, sm_scale):
    g = torch.Generator().manual_seed(1000 * Lq + Lk + D)
    q = torch.randn(2, heads[0], Lq, D, generator=g).to(dtype)
    k = (torch.randn(2, heads[1], Lk, D, generator=g) + 0.5).to(dtype)
    v = torch.randn(2, heads[1], Lk, D, generator=g).to(dtype)
    _hold(*_run(q, k, v, causal, layout, smooth_k, sm_scale), dtype)


@pytest.mark.parametrize("causal", [False, True])
def test_hd256_scores_at_the_int32_extreme(causal):
    """q = +c in every channel, k = +c / -c alternating over the keys, no smoothing: every INT32 score is +-127 * 127 * 256 = +-4 129 024, beyond
    the +-2^21 the D <= 128 kernels' score conversion is exact for."""
    c, g = 96.0, torch.Generator().manual_seed(7)
    q = torch.full((2, 2, 33, 256), c).half()
    k = (torch.full((2, 2, 65, 256), c) * torch.tensor([1.0, -1.0]).repeat(33)[:65, None]).half()
    v = torch.randn(2, 2, 65, 256, generator=g).half()
    _hold(*_run(q, k, v, causal, "HND", False, 1e-4), F16)       # (a small sm_scale keeps the LSE where FP32 resolves the bar)
