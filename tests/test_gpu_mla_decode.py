"""GPU: ``sageattention_amd.mla_decode.sageattn_mla_decode`` (FP8-PV attention for the absorbed MLA decode shape: 576-wide Q / K rows of one shared
latent, V its first 512 channels) against a CPU restatement composed from tests/ref_fp8_torch.py and against FP64 softmax attention.

The restatement, per sample: ``quant_int8_per_thread`` on the valid rows with ``groups(len, "per_thread", "k")`` and the mean; ``quant_v_fp8`` on
``kv[:len, :512]`` zero-padded to 576; the query rows of a position through ``quant_int8_per_thread`` with every row its own group; then per query
position ``attn_fp8(causal=False, two_level=True)`` on the first ``len - Lq + i + 1`` keys of the ALREADY quantised K and V.  Its output is sliced
to 512 before any reduction (the padded channels are NaN: a zero V scale).

Bar (the project's for every default route): |o - restatement| <= 2e-3 max|o| + one output ulp at max|o|; |lse - restatement's| <= 5e-3, with the
FP32 correction q . mean sm_scale added to the restatement's LSE.  Anchor: the kernel's error against FP64 may exceed the restatement's own by no
more than that bar.  A position in front of key 0 must give exactly o = +0 and lse = -inf.  Each case is the smallest shape that reaches one
mechanism of the kernel (64-key tiles, two-slot rings, 128-row blocks, four waves of 32 rows, rows that straddle positions)."""
import math

import pytest
import torch
import torch.nn.functional as F

import util  # noqa: F401  (sys.path)
import ref_fp8_torch as ref

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DEV = torch.device("cuda:0")
# (Lq, Hq, kv_lens, Lk, dtype, smooth_k, sm_scale)
CASES = [
    (1, 1, [1, 1], 1, F16, True, None),                 # minimal call
    (1, 16, [65, 33], 65, BF16, True, None),            # partial wave, ragged second tile, per-sample lengths
    (1, 128, [64, 64], 64, F16, False, None),           # one block, one tile
    (1, 128, [192, 129], 192, BF16, True, 0.05),        # the rings wrap
    (2, 128, [449, 257], 449, BF16, True, None),        # second row block, steady state, position 0 one key short
    (3, 48, [200, 70], 200, F16, True, 0.03),           # 144 rows: a block holds two positions, a limit inside a tile
    (4, 16, [2, 0], 64, BF16, True, None),              # positions in front of key 0 and a keyless sample: exact +0 / -inf
    (1, 128, [63, 64], 64, BF16, True, None),           # a full block of heads, the last key on either side of the first tile boundary ...
    (1, 128, [65, 127], 127, F16, True, None),
    (1, 128, [128, 129], 129, BF16, False, None),       # ... and of the second
    (8, 16, [200, 70], 200, F16, True, None),           # Lq 8, the documented upper end: one block of eight positions
    (8, 32, [129, 7], 129, BF16, True, None),           # two blocks; fewer keys than positions: position 0 of sample 1 in front of key 0
]


def _references(q, kv, lens, sm, smooth_k):
    """(restatement o, restatement lse, FP64 o) on CPU: o [B, Lq, Hq, 512] and the natural-log lse [B, Hq, Lq], FP64; +0 / -inf without a key."""
    B, Lq, Hq, _ = q.shape
    ro, to = torch.zeros(B, Lq, Hq, 512, dtype=torch.float64), torch.zeros(B, Lq, Hq, 512, dtype=torch.float64)
    rlse = torch.full((B, Hq, Lq), -math.inf, dtype=torch.float64)
    own = torch.arange(Hq)                                                      # every query row its own scale group
    for b, n in enumerate(lens):
        if n == 0:
            continue
        k = kv[b, :n]
        km = k.float().mean(dim=0).to(k.dtype) if smooth_k else None
        gk, nk = ref.groups(n, "per_thread", "k")
        k8, ks = ref.quant_int8_per_thread(k, gk, nk, mean=km)
        v8, vs, _ = ref.quant_v_fp8(F.pad(k[:, :512], (0, 64)), False)
        for i in range(Lq):
            vis = n - Lq + i + 1
            if vis <= 0:
                continue
            q8, qs = ref.quant_int8_per_thread(q[b, i], own, Hq)
            o, lse = ref.attn_fp8(q8, k8[:vis], v8[:vis], qs, own, ks, gk[:vis], vs, None, causal=False, sm_scale=sm, two_level=True,
                                  out_dtype=q.dtype)
            ro[b, i] = o[:, :512].double()
            rlse[b, :, i] = lse.double() / ref.LOG2E + ((q[b, i].double() * km.double()).sum(-1) * sm if smooth_k else 0.0)
            s = q[b, i].double() @ k[:vis].double().T * sm
            to[b, i] = torch.softmax(s, dim=-1) @ k[:vis, :512].double()
    return ro, rlse, to


def _hold(o, lse, refs, dtype):
    ro, rlse, to = refs
    o, lse = o.cpu().double(), lse.cpu().double()
    scale = ro.abs().max().item()
    bar = 2e-3 * scale + (2.0 ** -10 if dtype == F16 else 2.0 ** -7) * scale
    seen = torch.isfinite(rlse)                                                 # [B, Hq, Lq]: rows that see a key
    err, err_k, err_r = (o - ro).abs().max().item(), (o - to).abs().max().item(), (ro - to).abs().max().item()
    lse_err = (lse - rlse)[seen].abs().max().item() if seen.any() else 0.0
    print(f"max|o| {scale:.3e} bar {bar:.3e} | kernel-restatement {err:.3e} | kernel-fp64 {err_k:.3e} restatement-fp64 {err_r:.3e} | lse {lse_err:.3e}")
    assert torch.isfinite(o).all() and torch.isfinite(ro).all()
    assert torch.equal(torch.isfinite(lse), seen) and (lse[~seen] == -math.inf).all()
    blind = ~seen.transpose(1, 2)                                               # [B, Lq, Hq]
    assert (o[blind] == 0).all() and not torch.signbit(o[blind]).any()
    assert err <= bar
    assert err_k <= err_r + bar
    assert lse_err <= 5e-3


def _inputs(Lq, Hq, Lk, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(2, Lq, Hq, 576, generator=g).to(dtype)
    kv = (torch.randn(2, Lk, 576, generator=g) + 0.5).to(dtype)
    return q, kv


def _call(q, kv, lens, **kw):
    from sageattention_amd.mla_decode import sageattn_mla_decode
    out = sageattn_mla_decode(q.to(DEV), kv.to(DEV) if isinstance(kv, torch.Tensor) else kv,
                              None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV), return_lse=True, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("Lq,Hq,lens,Lk,dtype,smooth_k,sm_scale", CASES)
def test_mla_decode_matches_the_restatement_and_fp64(Lq, Hq, lens, Lk, dtype, smooth_k, sm_scale):
    q, kv = _inputs(Lq, Hq, Lk, dtype, 1000 * Lq + Hq + Lk)
    o, lse = _call(q, kv, lens, sm_scale=sm_scale, smooth_k=smooth_k)
    assert o.dtype == dtype and o.shape == (2, Lq, Hq, 512) and lse.shape == (2, Hq, Lq) and lse.dtype == torch.float32
    _hold(o, lse, _references(q, kv, lens, 576 ** -0.5 if sm_scale is None else sm_scale, smooth_k), dtype)


def test_rows_past_the_lengths_are_never_read():
    q, kv = _inputs(1, 32, 449, BF16, 5)
    lens = [100, 5]
    poisoned = kv.clone()
    for b, n in enumerate(lens):
        poisoned[b, n:] = math.nan
    o, lse = _call(q, poisoned, lens)
    o_cut, lse_cut = _call(q, kv[:, :100].contiguous(), lens)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    assert torch.equal(o, o_cut) and torch.equal(lse, lse_cut)


def test_quantise_once_and_strided_q():
    from sageattention_amd.mla_decode import mla_quantize_latent, sageattn_mla_decode
    q, kv = _inputs(2, 48, 200, F16, 6)
    lens = torch.tensor([200, 70], dtype=torch.int32, device=DEV)
    o, lse = _call(q, kv, [200, 70])
    lat = mla_quantize_latent(kv.to(DEV), lens)
    o1, lse1 = sageattn_mla_decode(q.to(DEV), lat, return_lse=True)
    big = torch.zeros(2, 3, 56, 640, dtype=F16, device=DEV)                      # q as a view of a larger tensor: every stride differs
    big[:, :2, 8:, 64:] = q.to(DEV)
    o2, lse2 = sageattn_mla_decode(big[:, :2, 8:, 64:], lat, return_lse=True)
    torch.cuda.synchronize()
    for a, b in ((o1, lse1), (o2, lse2)):
        assert torch.equal(a, o) and torch.equal(b, lse)


def test_mla_decode_scores_at_the_int32_extreme():
    """q = +c in every channel, k = +c / -c alternating over the keys, no smoothing: every INT32 score is +-127 * 127 * 576 = +-9 290 304, beyond
    the +-2^21 the D <= 128 kernels' score conversion is exact for and below the 2^24 v_cvt_f32_i32 takes exactly."""
    c, lens = 96.0, [65, 33]
    q = torch.full((2, 1, 16, 576), c).half()
    kv = (torch.full((2, 65, 576), c) * torch.tensor([1.0, -1.0]).repeat(33)[:65, None]).half()
    o, lse = _call(q, kv, lens, sm_scale=3e-5, smooth_k=False)            # (a small sm_scale keeps the LSE where FP32 resolves the bar)
    _hold(o, lse, _references(q, kv, lens, 3e-5, False), F16)
