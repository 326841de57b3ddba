"""GPU: ``sageattn_mla_decode(..., num_splits=S)``, the exact split of the key range for the absorbed MLA decode call (DESIGN 3.30,
include/sage_mlasplit_gfx950.h): every work item as S chunks of ``T = ceil(ceil(Lk / 64) / S)`` tiles, every P the unsplit call's.

Each case of ``CASES`` is the smallest shape that reaches one mechanism of the chunking and is held to three checks: (1) ``_hold`` of
tests/test_gpu_mla_decode.py against the restatement and FP64 at the project's bars; (2) ``_assert_matches_unsplit`` of
tests/test_gpu_split_exact.py against the same call without the keyword (two output ulps + 1e-5 max, rel-RMS 1e-3, LSE 1e-5; ``-inf`` where and
only where the unsplit call has it); (3) the call on an ``MlaLatent`` bit for bit the call on ``kv``.  An UNSEEDED split would pass all three:
what holds "exact" is ``test_pass_1_writes_the_loops_own_maxima``, which compares ``chunk_max`` bit for bit with a restatement -- the seeds
are the loop's own running maxima or they are not."""
import math

import pytest
import torch

import util  # noqa: F401  (sys.path)
import ref_fp8_torch as ref
import test_gpu_fence as fence_base
from test_gpu_fence import In, run_fenced
from test_gpu_fence_wide import PoisonedKV, WideFence
from test_gpu_mla_decode import _call, _hold, _inputs, _references
from test_gpu_split_exact import _assert_matches_unsplit

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DEV = torch.device("cuda:0")
# (Lq, Hq, kv_lens, Lk, S, dtype, smooth_k, sm_scale)
CASES = [
    (1, 128, [449, 257], 449, 4, BF16, True, None),     # T 2; sample 1 ends with one key in chunk 2, its chunk 3 is empty
    (2, 128, [449, 257], 449, 3, F16, True, None),      # T 3: chunks of 3, 3, 2 tiles, the ring wraps inside a chunk; two row blocks
    (3, 48, [130, 66], 200, 2, BF16, True, None),       # the boundary at key 128 between one block's positions; a 16-row last block; empty chunk
    (1, 16, [129, 7], 129, 4, F16, True, None),         # T 1; chunk 3 lies past the tensor; a partial wave
    (4, 16, [2, 0], 64, 2, BF16, True, None),           # positions in front of key 0, a keyless sample: exact +0 / -inf
    (8, 32, [321, 64], 321, 2, F16, False, 0.05),
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _matches_unsplit(split, unsplit, dtype, desc):
    (o, lse), (o0, lse0) = split, unsplit
    blind = torch.isinf(lse0)
    assert torch.equal(torch.isinf(lse), blind) and bool((lse[blind] == -math.inf).all()), desc         # -inf matches -inf ...
    _assert_matches_unsplit(o, lse.masked_fill(blind, 0.0), o0, lse0.masked_fill(blind, 0.0), 0 if dtype == F16 else 1, desc)


@pytest.mark.parametrize("Lq,Hq,lens,Lk,S,dtype,smooth_k,sm_scale", CASES)
def test_split_against_the_references_the_unsplit_call_and_the_latent(Lq, Hq, lens, Lk, S, dtype, smooth_k, sm_scale):
    from sageattention_amd.mla_decode import mla_quantize_latent
    q, kv = _inputs(Lq, Hq, Lk, dtype, 1000 * Lq + Hq + Lk + S)
    kw = dict(sm_scale=sm_scale, smooth_k=smooth_k)
    o, lse = _call(q, kv, lens, num_splits=S, **kw)
    assert o.dtype == dtype and o.shape == (2, Lq, Hq, 512) and lse.shape == (2, Hq, Lq) and lse.dtype == torch.float32
    _hold(o, lse, _references(q, kv, lens, 576 ** -0.5 if sm_scale is None else sm_scale, smooth_k), dtype)
    _matches_unsplit((o, lse), _call(q, kv, lens, **kw), dtype, (Lq, Hq, lens, Lk, S))
    lat = mla_quantize_latent(kv.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), smooth_k)
    o1, lse1 = _call(q, lat, None, num_splits=S, sm_scale=sm_scale)
    assert torch.equal(o1, o) and torch.equal(lse1, lse)


@pytest.mark.parametrize("rising", [True, False])
def test_seeds_below_and_above_the_chunks_own_maximum(rising):
    """T 1, eight chunks, key rows scaled by a factor that rises (falls) 64-fold along the sequence: every chunk's seed lies below (above) the
    maximum of its own keys, so m moves inside every chunk (never moves after chunk 0)."""
    q, kv = _inputs(1, 128, 449, BF16, 77)
    factor = 64.0 ** (torch.arange(449) / 448.0)
    kv = (kv.float() * (factor if rising else factor.flip(0))[None, :, None]).to(BF16)
    _matches_unsplit(_call(q, kv, [449, 449], num_splits=8), _call(q, kv, [449, 449]), BF16, rising)


@pytest.mark.parametrize("Lq,Hq,lens,Lk,S,dtype,smooth_k,sm_scale", [CASES[0], CASES[2]])
def test_pass_1_writes_the_loops_own_maxima(Lq, Hq, lens, Lk, S, dtype, smooth_k, sm_scale):
    """``chunk_max`` of a call through the binding, on a workspace the test owns, bit for bit: exact integer scores of the quantised q and K,
    ``m = float32(float64(s) * float64(cs) - offset)`` (the product of two FP32 numbers is exact in FP64: one rounding, an fma) with
    ``cs = sm_scale_log2 * (q_scale * k_scale)``, the maximum over the keys of the chunk that the row sees, ``-inf`` where it sees none.  (The
    fma is monotone in s, so its maximum over a K-scale group is the fma of the group's integer maximum, which is how the kernel forms it.)"""
    from sageattention_amd import _cabi, _cabi_mlasplit
    from sageattention_amd.mla_decode import mla_quantize_latent
    from sageattention_amd.quant import _p, _stream
    q, kv = _inputs(Lq, Hq, Lk, dtype, 1000 * Lq + Hq + Lk + S)
    qd = q.to(DEV)
    lat = mla_quantize_latent(kv.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), smooth_k)
    lib, R, T = _cabi_mlasplit.load(), Lq * Hq, ((Lk + 63) // 64 + S - 1) // S
    ws_bytes = lib.sage_mlasplit_ws_bytes(2, Lq, Hq, S)
    ws = torch.full((ws_bytes // 4,), math.nan, dtype=torch.float32, device=DEV)
    o, lse = torch.empty(2, Lq, Hq, 512, dtype=dtype, device=DEV), torch.empty(2, Hq, Lq, dtype=torch.float32, device=DEV)
    sm = 576 ** -0.5 if sm_scale is None else sm_scale
    rc = lib.sage_mlasplit_attn(_p(qd), _p(lat.k_img), _p(lat.v_img), _p(lat.k_scale), _p(lat.v_scale), _p(lat.kv_lens), _p(o), _p(lse), 2, Lq, Hq,
                                Lk, 576, 512, qd.stride(0), qd.stride(1), qd.stride(2), float(sm), 0 if dtype == F16 else 1, _stream(qd), S,
                                _p(ws), ws_bytes)
    _cabi.check(rc, "sage_mlasplit_attn")
    torch.cuda.synchronize()
    got = ws[:2 * S * R].view(2, S, R).cpu()
    want = torch.full((2, S, Lq, Hq), -math.inf)
    sm2 = torch.tensor(sm, dtype=torch.float32) * torch.tensor(ref.LOG2E, dtype=torch.float32)
    own, mean = torch.arange(Hq), lat.k_mean.cpu()
    for b, n in enumerate(lens):
        gk, nk = ref.groups(n, "per_thread", "k")
        k8, ks = ref.quant_int8_per_thread(kv[b, :n], gk, nk, mean=mean[b] if smooth_k else None)
        for i in range(Lq):
            q8, qs = ref.quant_int8_per_thread(q[b, i], own, Hq)
            m = ref._fma32((q8.double() @ k8.double().T).float(), sm2 * (qs[:, None] * ks[gk][None, :]), -ref.S_FP8_OFFSET)     # [Hq, n]
            for c in range(S):
                lo, hi = 64 * T * c, min(64 * T * (c + 1), n - Lq + i + 1)
                if hi > lo:
                    want[b, c, i] = m[:, lo:hi].amax(dim=1)
    want = want.view(2, S, R)
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and not bool(got.isnan().any())
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} maxima differ, by up to {(got - want).nan_to_num().abs().max():.3e}"


@pytest.mark.parametrize("Lq,Hq,lens,Lk,S,dtype,smooth_k,sm_scale", [CASES[0], CASES[2]])
def test_split_inside_the_fence(Lq, Hq, lens, Lk, S, dtype, smooth_k, sm_scale, monkeypatch):
    """Both fills; workspace, images and outputs between guards and poisoned.  Both cases have empty chunks, whose ``o_part`` is the fill (NaN
    under 0xFF) and must stay out of ``o``: the result is the plain run's, bit for bit, and finite."""
    from sageattention_amd.mla_decode import sageattn_mla_decode
    monkeypatch.setattr(fence_base, "Fence", WideFence)
    q, kv = _inputs(Lq, Hq, Lk, dtype, 1000 * Lq + Hq + Lk + S)
    seen = run_fenced(lambda q, kv, kv_lens: sageattn_mla_decode(q, kv, kv_lens, return_lse=True, num_splits=S),
                      [In(q), PoisonedKV(kv, lens), In(torch.tensor(lens, dtype=torch.int32))])
    ws_floats = 2 * (-(-2 * S * Lq * Hq * 4 // 128) * 32) + 2 * S * Lq * Hq * 512
    assert ("sageattn_mla_decode", (ws_floats,), torch.float32) in seen.allocs, sorted(seen.allocs, key=str)


def test_split_call_replays_from_a_graph():
    """Captured once with ``num_splits=4``, replayed after the CONTENTS of ``kv_lens`` changed: the grids come from the shapes, the lengths are
    read on the device.  Each replay is the eager call on the same lengths, bit for bit."""
    from sageattention_amd.mla_decode import mla_quantize_latent, sageattn_mla_decode
    q, kv = _inputs(1, 128, 449, BF16, 9)
    qd, lens = q.to(DEV), torch.tensor([449, 257], dtype=torch.int32, device=DEV)
    lat = mla_quantize_latent(kv.to(DEV), lens)
    sageattn_mla_decode(qd, lat, return_lse=True, num_splits=4)            # (warm-up: library load and the LDS opt-in happen outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = sageattn_mla_decode(qd, lat, return_lse=True, num_splits=4)
    for new in ([449, 257], [130, 200], [64, 0]):                          # (never past what the images were written for)
        lens.copy_(torch.tensor(new, dtype=torch.int32))
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        o0, lse0 = sageattn_mla_decode(qd, lat, return_lse=True, num_splits=4)
        torch.cuda.synchronize()
        assert torch.equal(o, o0) and torch.equal(lse, lse0), new
