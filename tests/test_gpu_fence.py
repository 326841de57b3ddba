"""GPU: every route inside guarded, poisoned memory (tests/fence.py).

The rest of the suite holds every route's arithmetic to the oracle; this file holds the ADDRESS arithmetic.  One pattern per case:

  1. q, k, v are built on the CPU from a seeded generator (K with a per-channel bias);
  2. the call runs plainly and its results are kept;
  3. for each fill byte (0xFF: NaN / -1, 0x5A: finite) the same call runs with its inputs placed by the fence and the fence active, so
     every buffer the package allocates (quantised operands, scales, V images, workspaces, partials, outputs) lies between two 64 KiB guards
     and starts out as poison;
  4. outputs and LSE are bit-identical to the plain run and finite (an LSE is -inf by contract for rows without a key -- packed calls with an
     empty key side -- and only there); no guard byte changed; the fence recorded allocations made from inside ``sageattention_amd`` and
     the returned output lives in one of its arenas (so a refactor to another allocation function fails here instead of going vacuous).

No tolerance appears anywhere: every comparison is bit equality.

Not fenced: what torch allocates itself -- for padded head dims (40, 96) the library pads with ``F.pad``, and those padded copies of q / k / v
are torch's own allocations; ``.contiguous()`` / ``.to()`` copies and the LSE unit conversion likewise.  Temporaries and outputs of those calls
still are.  With ``gap`` > 0 the inputs are views with guard rows behind EVERY head (NHD: every batch; strides stay multiples of 8), and the plain run
gets inputs of the same strides, so both runs take the same route.  Where a case asks for a route (``v_in_place``, ``fused_prepass``, a split, a
mask, the plan), the allocations recorded by the fence must show that it ran: those switches fall back silently when a precondition fails.

ROUTES is the set of public names that have fenced cases; a test compares it with ``sageattention_amd.__all__``.
"""
import ctypes

import numpy as np
import pytest
import torch

from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, core as sc, kernel_api, ops as sa_ops, quant as sq, ring
    DEV = torch.device("cuda:0")

F16, BF16 = torch.float16, torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


# ------------------------------------------------------------------------------------------------ the pattern
class In:
    """A caller tensor (built on the CPU) and how it is placed: ``gap`` guard rows behind every head (HND) or every batch's block (NHD) of a dense 4-D tensor."""

    def __init__(self, t, gap=0, layout="HND"):
        self.t, self.gap, self.layout = t, gap, layout

    def plain(self):
        if not self.gap:
            return self.t.to(DEV)
        seq = 2 if self.layout == "HND" else 1
        full = list(self.t.shape)
        full[seq] += self.gap
        buf = torch.zeros(full, dtype=self.t.dtype, device=DEV)
        view = buf.narrow(seq, 0, self.t.shape[seq])
        view.copy_(self.t)
        return view

    def fenced(self, f):
        return f.input(self.t, self.gap, self.layout)


def _tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


class Seen:
    """What the fences of one case recorded from inside the package: allocation sites (file:line), allocating functions and
    (function, shape, dtype) of every allocation.  Which route ran shows in what it allocated: ``v_image16`` -- an fp16 V tile image
    ``[.., D, 64]`` was built, i.e. V was NOT read in place."""

    def __init__(self):
        self.sites, self.funcs, self.allocs = set(), set(), set()

    def add(self, f):
        self.sites |= set(f.package_sites())
        self.allocs |= set(f.package_allocations())
        self.funcs |= {a[0] for a in f.package_allocations()}

    @property
    def v_image16(self):
        return any(dt == F16 and len(shape) >= 4 and shape[-1] == 64 for fn, shape, dt in self.allocs
                   if fn in ("prep_v_fp16", "prep_v_fp16_varlen", "prepass_kv_fp8", "prepass_kv_varlen"))


def run_fenced(call, inputs, lse_neg_inf_ok=False):
    """Steps 2-4 of the module docstring for ``call(*device tensors) -> o | (o, lse)``.  Returns what the fences saw (``Seen``)."""
    want = _tuple(call(*[i.plain() for i in inputs]))
    torch.cuda.synchronize()
    want = tuple(w.clone() for w in want)
    seen = Seen()
    for fill in FILLS:
        with Fence(fill) as f:
            got = _tuple(call(*[i.fenced(f) for i in inputs]))
            f.check()
            tag = f"fill 0x{fill:02X}"
            assert f.package_sites(), f"{tag}: no allocation from inside sageattention_amd went through the fence"
            assert f.owns(got[0]), f"{tag}: the returned output does not live in a fenced arena"
            assert len(got) == len(want)
            for i, (g, w) in enumerate(zip(got, want)):
                assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), \
                    f"{tag}: result {i} differs from the plain run in {int((g != w).sum())} of {g.numel()} elements"
            assert bool(torch.isfinite(got[0].float()).all()), f"{tag}: the output is not finite"
            for lse in got[1:]:
                if lse_neg_inf_ok:
                    assert not bool(lse.isnan().any()) and not bool((lse == float("inf")).any()), f"{tag}: NaN / +inf in the LSE"
                else:
                    assert bool(torch.isfinite(lse).all()), f"{tag}: the LSE is not finite"
            seen.add(f)
    return seen


def qkv(B, Hq, Hkv, Lq, Lk, D, dtype, seed, layout="HND", gap=0):
    """As ``rand_qkv(..., kbias=1.0)`` of test_gpu_parity.py, in ``layout``, as ``In``s."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Hq, Lq, D, generator=g).to(dtype)
    k = (torch.randn(B, Hkv, Lk, D, generator=g) + 1.0 * torch.randn(1, Hkv, 1, D, generator=g)).to(dtype)
    v = torch.randn(B, Hkv, Lk, D, generator=g).to(dtype)
    if layout == "NHD":
        q, k, v = (t.transpose(1, 2).contiguous() for t in (q, k, v))
    return [In(t, gap, layout) for t in (q, k, v)]


# ------------------------------------------------------------------------------------------------ dense shapes  (B, Hq, Hkv, Lq, Lk)
def shapes_matrix(causal):
    """Per head dim and PV type: Lk = 63, 64, 65, a cross shape, a ragged query and key side, one length >= 2138 (the pipelined steady state,
    its last-tile bodies and the ragged tail all run).  Causal calls need Lq = Lk."""
    if causal:
        return [(2, 4, 2, 63, 63), (1, 2, 2, 64, 64), (1, 2, 1, 65, 65), (1, 4, 2, 333, 333), (1, 2, 1, 2203, 2203)]
    return [(2, 4, 2, 200, 63), (1, 2, 2, 100, 64), (1, 2, 1, 129, 65), (1, 4, 2, 300, 333), (1, 2, 1, 130, 2203)]


def shapes_route(causal):
    """What every route sees at least: a ragged query side, a ragged key side, Lk < 64."""
    return [(2, 4, 2, 63, 63), (1, 4, 2, 333, 333)] if causal else [(2, 4, 2, 200, 63), (1, 4, 2, 300, 333)]


DENSE = []      # (id, public name, (B, Hq, Hkv, Lq, Lk), D, dtype, layout, gap, kwargs)


def _add(name, shapes, D, dtype, layout, kw, gap=0, tag=""):
    for s in shapes:
        cid = f"{name.replace('sageattn_qk_int8_', '')}{'-' + tag if tag else ''}-{'c' if kw.get('is_causal') else 'nc'}-b{s[0]}h{s[1]}k{s[2]}q{s[3]}l{s[4]}" \
              f"d{D}-{'f16' if dtype == F16 else 'bf16'}-{layout}{'-gap' + str(gap) if gap else ''}"
        DENSE.append(pytest.param(name, s, D, dtype, layout, gap, kw, id=cid))


def _alt(i):
    """Alternate head dim, dtype and layout over the variants of a route."""
    return (64, 128)[i % 2], (F16, BF16)[(i // 2) % 2], ("HND", "NHD")[(i + i // 2) % 2]


# default FP8 route: sageattn, causal and not, fp16 and bf16, HND and NHD, GQA; the whole matrix at D = 64 / 128, padded head dims 40 / 96
for causal in (False, True):
    for D in (64, 128):
        for dtype, layout in ((F16, "HND"), (BF16, "NHD")):
            _add("sageattn", shapes_matrix(causal), D, dtype, layout, dict(is_causal=causal, return_lse=True))
    for D, dtype, layout in ((40, F16, "NHD"), (96, BF16, "HND")):
        _add("sageattn", shapes_route(causal), D, dtype, layout, dict(is_causal=causal, return_lse=True))
    for D, dtype, layout in ((64, BF16, "HND"), (128, F16, "NHD")):
        _add("sageattn", shapes_route(causal), D, dtype, layout, dict(is_causal=causal), gap=8)

# sageattn_qk_int8_pv_fp8_cuda
FP8_VARIANTS = [
    ("per_block", dict(qk_quant_gran="per_block")), ("per_warp", dict(qk_quant_gran="per_warp")), ("per_thread", dict(qk_quant_gran="per_thread")),
    ("acc_fp32", dict(pv_accum_dtype="fp32")), ("acc_fp32fp32", dict(pv_accum_dtype="fp32+fp32")), ("acc_fp32fp16", dict(pv_accum_dtype="fp32+fp16")),
    ("int8q", dict(fuse_q_quant=False)), ("folded", dict(fp8_scores="folded")), ("folded_int8q", dict(fp8_scores="folded", fuse_q_quant=False)),
    ("smooth_v", dict(pv_accum_dtype="fp32", smooth_v=True)), ("prepass_fused", dict(fused_prepass=True)), ("prepass_seq", dict(fused_prepass=False)),
    ("no_smooth_k", dict(smooth_k=False)),
]
for i, (tag, kw) in enumerate(FP8_VARIANTS):
    D, dtype, layout = _alt(i)
    for causal in (False, True):
        _add("sageattn_qk_int8_pv_fp8_cuda", shapes_route(causal), D, dtype, layout, dict(kw, is_causal=causal, return_lse=True), tag=tag)
for D, dtype, layout in ((64, F16, "NHD"), (128, BF16, "HND")):
    # split_kv = 4 divides whole 64-key tiles only (Lk = 512; the ragged key side of this route is the exact split's, below)
    _add("sageattn_qk_int8_pv_fp8_cuda", [(1, 4, 2, 200, 512)], D, dtype, layout, dict(split_kv=4, return_lse=True), tag="split4")
    _add("sageattn_qk_int8_pv_fp8_cuda", [(1, 4, 2, 512, 512)], D, dtype, layout, dict(split_kv=4, is_causal=True, return_lse=True), tag="split4")
    # the exact split: without and with a ragged tail chunk (Lk = 512 / 555, Lk < 128: one tile + tail), causal with an odd chunk count
    _add("sageattn_qk_int8_pv_fp8_cuda", [(1, 4, 2, 200, 512), (1, 4, 2, 200, 555)], D, dtype, layout,
         dict(split_kv_exact=True, split_kv=2 if D == 64 else 4, return_lse=True), tag="exact")
    _add("sageattn_qk_int8_pv_fp8_cuda", [(1, 2, 2, 100, 191), (2, 2, 1, 130, 2203)], D, dtype, layout,
         dict(split_kv_exact=True, split_kv=2, return_lse=True), tag="exact")
    _add("sageattn_qk_int8_pv_fp8_cuda", [(1, 4, 2, 333, 333)], D, dtype, layout, dict(split_kv_exact=True, split_kv=5, is_causal=True, return_lse=True),
         tag="exact")
_add("sageattn_qk_int8_pv_fp8_cuda", [(1, 2, 1, 100, 4096 + 37)], 128, BF16, "HND", dict(split_kv_exact=True, return_lse=True), tag="exact_auto")

# sageattn_qk_int8_pv_fp8_cuda_sm90
for i, gran in enumerate(("per_warp", "per_thread")):
    for D, dtype, layout in ((64, (F16, BF16)[i], "HND"), (128, (BF16, F16)[i], "NHD")):
        for causal in (False, True):
            _add("sageattn_qk_int8_pv_fp8_cuda_sm90", shapes_route(causal) + shapes_matrix(causal)[-1:], D, dtype, layout,
                 dict(qk_quant_gran=gran, is_causal=causal, return_lse=True), tag=gran)

# sageattn_qk_int8_pv_fp16_cuda: both forms of the V operand (rows in place / tile image) over the whole matrix, then the variants
for causal in (False, True):
    for D in (64, 128):
        for vip, layout in ((True, "HND"), (False, "NHD")) if D == 64 else ((True, "NHD"), (False, "HND")):
            _add("sageattn_qk_int8_pv_fp16_cuda", shapes_matrix(causal), D, F16, layout, dict(v_in_place=vip, is_causal=causal, return_lse=True),
                 tag="vrows" if vip else "image")
        for vip in (True, False):
            _add("sageattn_qk_int8_pv_fp16_cuda", shapes_route(causal), D, F16, "HND" if vip else "NHD", dict(v_in_place=vip, is_causal=causal), gap=8,
                 tag="vrows" if vip else "image")
FP16_VARIANTS = [
    ("acc_fp32", dict(pv_accum_dtype="fp32")), ("acc_fp16fp32", dict(pv_accum_dtype="fp16+fp32")), ("acc_fp16", dict(pv_accum_dtype="fp16")),
    ("smooth_v", dict(pv_accum_dtype="fp16", smooth_v=True)), ("int8q", dict(fuse_q_quant=False)), ("per_warp", dict(qk_quant_gran="per_warp")),
    ("per_block", dict(qk_quant_gran="per_block")), ("prepass_seq", dict(fused_prepass=False)),
]
for i, (tag, kw) in enumerate(FP16_VARIANTS):
    D, dtype, layout = _alt(i)                   # (bf16 inputs: always the tile image)
    for causal in (False, True):
        _add("sageattn_qk_int8_pv_fp16_cuda", shapes_route(causal), D, dtype, layout, dict(kw, is_causal=causal, return_lse=True), tag=tag)
_add("sageattn_qk_int8_pv_fp16_cuda", shapes_matrix(False), 64, BF16, "NHD", dict(return_lse=True), tag="bf16")
_add("sageattn_qk_int8_pv_fp16_cuda", shapes_matrix(True), 128, BF16, "HND", dict(is_causal=True, return_lse=True), tag="bf16")
# few queries against a long key range: the automatic split (S = 2 chunks of 32 tiles).  Like split_kv = 4 it divides whole 64-key tiles only
# (core._split_kv_plan returns 0 for Lk % 64 != 0), so this route cannot see a ragged key side or Lk < 64; its query side is ragged.
for D, dtype in ((64, F16), (128, BF16)):
    _add("sageattn_qk_int8_pv_fp16_cuda", [(1, 2, 1, 100, 4096)], D, dtype, "HND", dict(split_kv="auto", return_lse=True), tag="autosplit")

# sageattn_qk_int8_pv_fp16_triton (unmasked; the masked cases are below)
for i, (backend, vip) in enumerate((("triton", True), ("triton", False), ("cuda", None))):
    for D in (64, 128):
        layout = ("HND", "NHD")[(i + D // 64) % 2]
        for causal in (False, True):
            kw = dict(quantization_backend=backend, is_causal=causal, return_lse=True)
            if vip is not None:
                kw["v_in_place"] = vip
            tag = backend + ("" if vip is None else ("-vrows" if vip else "-image"))
            _add("sageattn_qk_int8_pv_fp16_triton", shapes_matrix(causal) if backend == "triton" else shapes_route(causal), D, F16, layout, kw, tag=tag)
            if backend == "triton":
                _add("sageattn_qk_int8_pv_fp16_triton", shapes_route(causal), D, F16, layout, dict(kw, return_lse=False), gap=8, tag=tag)
    _add("sageattn_qk_int8_pv_fp16_triton", shapes_route(False), 128 if i % 2 else 64, BF16, "NHD", dict(quantization_backend=backend, return_lse=True),
         tag=backend + "-bf16")


@pytest.mark.parametrize("name,shape,D,dtype,layout,gap,kw", DENSE)
def test_dense_routes_inside_the_fence(name, shape, D, dtype, layout, gap, kw):
    fn = getattr(sa, name)
    B, Hq, Hkv, Lq, Lk = shape
    ins = qkv(B, Hq, Hkv, Lq, Lk, D, dtype, seed=Lq + 3 * Lk + D, layout=layout, gap=gap)
    seen = run_fenced(lambda q, k, v: fn(q, k, v, tensor_layout=layout, **kw), ins)
    # the route asked for is the route that ran (the switches fall back silently when a precondition fails): it shows in what was allocated
    if kw.get("v_in_place") is not None:
        assert seen.v_image16 == (not kw["v_in_place"]), f"v_in_place={kw['v_in_place']}: {sorted(seen.funcs)}"
    if kw.get("fused_prepass") is not None:
        assert ("prepass_kv_fp8" in seen.funcs) == kw["fused_prepass"], f"fused_prepass={kw['fused_prepass']}: {sorted(seen.funcs)}"
    split = "_attn_fused_q_split_exact" if kw.get("split_kv_exact") else ("_attn_fused_q_split" if kw.get("split_kv") else None)
    assert {"_attn_fused_q_split_exact", "_attn_fused_q_split"} & seen.funcs == ({split} if split else set()), f"split route {split}: {sorted(seen.funcs)}"


# ------------------------------------------------------------------------------------------------ attn_mask
MASKED = []
for mi, mshape in enumerate(("LqLk", "B1LqLk", "1H1Lk")):
    for kind in ("bool", "add"):
        for (shape, D, dtype, layout, gap) in (((2, 4, 2, 200, 63), 64, F16, "HND", 0), ((1, 4, 2, 300, 333), 128, BF16, "NHD", 0),
                                               ((2, 4, 2, 129, 2203), (64, 128)[mi % 2], F16, "NHD", 0), ((2, 4, 2, 300, 333), (128, 64)[mi % 2], F16, "HND", 8)):
            if shape[4] == 2203 and (kind == "add") != (mi == 1):       # (one long case per mask shape)
                continue
            # (the quantisation backend does not change the masked attention launch: one backend for the long and the gapped shapes)
            for backend in ("triton",) if (gap or shape[4] == 2203) else ("triton", "cuda"):
                MASKED.append(pytest.param(mshape, kind, shape, D, dtype, layout, gap, backend,
                                           id=f"{mshape}-{kind}-b{shape[0]}q{shape[3]}l{shape[4]}d{D}-{layout}{'-gap8' if gap else ''}-{backend}"))


@pytest.mark.parametrize("mshape,kind,shape,D,dtype,layout,gap,backend", MASKED)
def test_masked_route_inside_the_fence(mshape, kind, shape, D, dtype, layout, gap, backend):
    """``sageattn_qk_int8_pv_fp16_triton(attn_mask=...)``: bool and additive masks in the broadcast shapes ``[Lq, Lk]``, ``[B, 1, Lq, Lk]`` and
    ``[1, Hq, 1, Lk]``, the mask tensors fenced as inputs too (the kernel reads them in place through zero strides).  Bool masks carry an
    all-False 128 x 64 tile (skipped by the kernel) where the key range has one; no row is fully masked, so every LSE is finite."""
    B, Hq, Hkv, Lq, Lk = shape
    ins = qkv(B, Hq, Hkv, Lq, Lk, D, dtype, seed=7 + Lq + Lk, layout=layout, gap=gap)
    ms = {"LqLk": (Lq, Lk), "B1LqLk": (B, 1, Lq, Lk), "1H1Lk": (1, Hq, 1, Lk)}[mshape]
    g = torch.Generator().manual_seed(Lq + Lk)
    if kind == "bool":
        m = torch.rand(ms, generator=g) < 0.7
        m[..., 0] = True                                   # (no fully masked row)
        if Lk >= 192 and mshape != "1H1Lk":
            m[..., :128, 64:128] = False
    else:
        m = (2.0 * torch.randn(ms, generator=g)).to(dtype)
    seen = run_fenced(lambda q, k, v, mask: sa.sageattn_qk_int8_pv_fp16_triton(q, k, v, tensor_layout=layout, attn_mask=mask,
                                                                               quantization_backend=backend, return_lse=True), ins + [In(m)])
    assert "_attn_masked" in seen.funcs and seen.v_image16, sorted(seen.funcs)


# ------------------------------------------------------------------------------------------------ packed batches
LENS = [1, 63, 64, 0, 65, 127, 129, 1000]
CROSS_Q, CROSS_K = [100, 1, 0, 300, 64, 5], [257, 64, 30, 129, 200, 0]        # an empty query side and an empty key side
LONG = [70, 2203, 1, 190]


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)


def packed(lq, lk, Hq, Hkv, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(int(sum(lq)), Hq, D, generator=g).to(dtype)
    k = (torch.randn(int(sum(lk)), Hkv, D, generator=g) + torch.randn(1, Hkv, D, generator=g)).to(dtype)
    v = torch.randn(int(sum(lk)), Hkv, D, generator=g).to(dtype)
    return [In(q), In(k), In(v), In(_cu(lq)), In(_cu(lk))]


VARLEN = []
for name in ("sageattn_varlen", "sageattn_qk_int8_pv_fp8_varlen"):
    short = "f16pv" if name == "sageattn_varlen" else "f8pv"
    for causal in (False, True):
        c = "c" if causal else "nc"
        for D, dtype in ((64, F16), (128, BF16), (40, BF16), (96, F16)):
            VARLEN.append(pytest.param(name, LENS, LENS, 4, 1, D, dtype, causal, {}, id=f"{short}-{c}-lens-d{D}"))
        for D, dtype in ((64, BF16), (128, F16)):
            VARLEN.append(pytest.param(name, CROSS_Q, CROSS_K, 4, 2, D, dtype, causal, {}, id=f"{short}-{c}-cross-d{D}"))
            VARLEN.append(pytest.param(name, LONG, LONG, 2, 1, D, dtype, causal, {}, id=f"{short}-{c}-long-d{D}"))
        for i, kw in enumerate((dict(fuse_q_quant=False), dict(work_list=False), dict(varlen_plan=False), dict(fused_prepass=False),
                                dict(fused_prepass=False, work_list=False, fuse_q_quant=False), dict(smooth_k=False))):
            D, dtype = ((64, F16), (128, BF16))[(i + causal) % 2]
            tag = "+".join(f"{a}={b}" for a, b in kw.items())
            VARLEN.append(pytest.param(name, LENS, LENS, 4, 2, D, dtype, causal, kw, id=f"{short}-{c}-{tag}-d{D}"))
            if i % 2 == causal:
                VARLEN.append(pytest.param(name, CROSS_Q, CROSS_K, 4, 2, D, dtype, causal, kw, id=f"{short}-{c}-{tag}-cross-d{D}"))
        VARLEN.append(pytest.param(name, "many", "many", 2, 1, 64, BF16, causal, {}, id=f"{short}-{c}-1100-sequences"))
    if short == "f8pv":
        VARLEN.append(pytest.param(name, LENS, LENS, 4, 2, 128, F16, False, dict(pv_accum_dtype="fp32"), id="f8pv-nc-acc_fp32-d128"))
        VARLEN.append(pytest.param(name, CROSS_Q, CROSS_K, 4, 2, 64, BF16, True, dict(pv_accum_dtype="fp32"), id="f8pv-c-acc_fp32-cross-d64"))


@pytest.mark.parametrize("name,lq,lk,Hq,Hkv,D,dtype,causal,kw", VARLEN)
def test_packed_routes_inside_the_fence(name, lq, lk, Hq, Hkv, D, dtype, causal, kw):
    """``sageattn_varlen`` and ``sageattn_qk_int8_pv_fp8_varlen`` (with its LSE): sequences side by side in one buffer, lengths around the tile
    edges, an empty sequence, ``cu_q != cu_k`` with an empty query side and an empty key side (rows without a key: zero output, LSE -inf), the
    route toggles, and more sequences than the plan takes."""
    if lq == "many":
        assert 1100 > _cabi.load().sage_varlen_plan_max_seqs()
        lq = lk = np.random.default_rng(3).integers(0, 40, size=1100)
        lq[7] = 130
    ins = packed(lq, lk, Hq, Hkv, D, dtype, seed=11 + D + causal)
    mq, mk = max(int(max(lq)), 1), max(int(max(lk)), 1)
    extra = dict(return_lse=True) if name == "sageattn_qk_int8_pv_fp8_varlen" else {}
    fn = getattr(sa, name)
    no_key = any(a > 0 and b == 0 for a, b in zip(lq, lk))          # rows without a key: their LSE is -inf by contract, and only theirs
    seen = run_fenced(lambda q, k, v, cu_q, cu_k: fn(q, k, v, cu_q, cu_k, mq, mk, is_causal=causal, **kw, **extra), ins, lse_neg_inf_ok=no_key)
    planned = kw.get("varlen_plan", True) and len(lq) <= 1024
    assert ("varlen_plan" in seen.funcs) == planned, sorted(seen.funcs)
    if kw.get("fused_prepass") is False or not planned:
        assert "prepass_kv_varlen" not in seen.funcs, sorted(seen.funcs)
    elif kw.get("smooth_k", True):
        assert "prepass_kv_varlen" in seen.funcs, sorted(seen.funcs)         # (the default route: the one-launch pre-pass)


# ------------------------------------------------------------------------------------------------ kernel-level entry points
@pytest.mark.parametrize("layout", ["HND", "NHD"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D,odt", [(64, F16), (128, BF16)])
def test_kernel_api_forward_inside_the_fence(D, odt, causal, layout):
    """``kernel_api.forward`` / ``forward_causal`` on operands from the library's own quantiser (which runs fenced too): V rows in place, and the
    masked form through the tile image."""
    for shape in shapes_route(causal) + shapes_matrix(causal)[-1:]:
        B, Hq, Hkv, Lq, Lk = shape
        ins = qkv(B, Hq, Hkv, Lq, Lk, D, F16, seed=5 + Lq + Lk, layout=layout)

        def call(q, k, v, mask=None):
            km = sq.channel_mean(k, layout).unsqueeze(2 if layout == "HND" else 1)
            q8, qs, k8, ks = sq.per_block_int8(q, k, km=km, tensor_layout=layout)
            if causal:
                return kernel_api.forward_causal(q8, k8, v, qs, ks, tensor_layout=layout, output_dtype=odt, return_lse=True)
            return kernel_api.forward(q8, k8, v, qs, ks, tensor_layout=layout, attn_mask=mask, output_dtype=odt, return_lse=True)

        seen = run_fenced(call, ins)
        assert not seen.v_image16, f"V was not read in place: {sorted(seen.funcs)}"
        if not causal and Lk == 333:
            g = torch.Generator().manual_seed(3)
            m = torch.rand((B, 1, Lq, Lk), generator=g) < 0.7
            m[..., 0] = True
            seen = run_fenced(call, ins + [In(m)])
            assert "_attn_masked" in seen.funcs and seen.v_image16, sorted(seen.funcs)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D,odt", [(64, BF16), (128, F16)])
def test_kernel_api_forward_varlen_inside_the_fence(D, odt, causal):
    for lq, lk in ((LENS, LENS), (CROSS_Q, CROSS_K)):
        ins = packed(lq, lk, 4, 2, D, F16, seed=17 + D)
        mq, mk = max(lq), max(lk)

        def call(q, k, v, cu_q, cu_k):
            q8, qs, k8, ks, cu_qs, cu_ks = kernel_api.per_block_int8_varlen_ref(q, k, cu_q, cu_k, mq, mk)
            return kernel_api.forward_varlen(q8, k8, v, cu_q, cu_k, mq, qs, ks, cu_qs, cu_ks, output_dtype=odt, is_causal=causal)

        run_fenced(call, ins)


# ------------------------------------------------------------------------------------------------ persistent route
@pytest.fixture
def forced_persistent(monkeypatch):
    probe = ctypes.c_int32(-1)
    monkeypatch.setattr(sa_ops, "_PERSISTENT", True)
    with sa_ops.launch_hooks(grid_probe=probe, force_persistent=True):
        yield probe


def test_persistent_dense_route_inside_the_fence(forced_persistent, monkeypatch):
    """The ticket-queue route, forced from two rounds of workgroups up: a dense non-causal call of 8 x 129 = 1032 query blocks, ragged on both
    sides.  The plain run is the ORDINARY launch; the probe shows that the fenced runs took the ticket route (fewer workgroups than items), whose
    counter block is allocated -- zeroed -- under the fence."""
    probe = forced_persistent
    B, H, L, D = 1, 8, 16384 + 37, 128
    items = B * H * ((L + 127) // 128)
    ins = qkv(B, H, H, L, L, D, BF16, seed=29)
    seen = []

    def call(q, k, v):
        probe.value = -1
        out = sa.sageattn(q, k, v, return_lse=True)
        seen.append(probe.value)
        return out

    monkeypatch.setattr(sa_ops, "_PERSISTENT", False)
    want = call(*[i.plain() for i in ins])
    assert seen == [items]
    monkeypatch.setattr(sa_ops, "_PERSISTENT", True)
    sites = run_fenced(call, ins).sites
    assert len(seen) == 4 and all(0 < n < items for n in seen[1:]), (seen, items)       # (run_fenced's own plain run is persistent too)
    assert any("_stream_cache.py" in s for s in sites), "the ticket block was not allocated under the fence"
    with Fence(0x5A) as f:                        # and against the ordinary launch
        got = call(*[i.fenced(f) for i in ins])
        f.check()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("name", ["sageattn_varlen", "sageattn_qk_int8_pv_fp8_varlen"])
def test_persistent_packed_causal_route_inside_the_fence(forced_persistent, monkeypatch, name):
    probe = forced_persistent
    lens = [4096, 1, 640, 129, 3000, 64, 1500, 777, 2100]
    ins = packed(lens, lens, 16, 4, 128, BF16, seed=23)
    fn = getattr(sa, name)
    seen = []

    def call(q, k, v, cu_q, cu_k):
        probe.value = -1
        out = fn(q, k, v, cu_q, cu_k, max(lens), max(lens), is_causal=True)
        seen.append(probe.value)
        return out

    monkeypatch.setattr(sa_ops, "_PERSISTENT", False)
    want = call(*[i.plain() for i in ins])
    ordinary = seen[0]
    monkeypatch.setattr(sa_ops, "_PERSISTENT", True)
    sites = run_fenced(call, ins).sites
    assert len(seen) == 4 and all(0 < n < ordinary for n in seen[1:]), (seen, ordinary)
    assert any("_stream_cache.py" in s for s in sites), "the ticket block was not allocated under the fence"
    with Fence(0xFF) as f:
        got = call(*[i.fenced(f) for i in ins])
        f.check()
        assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ ring step
@pytest.mark.parametrize("causal", [False, True])
def test_ring_steps_on_one_gpu_inside_the_fence(causal):
    """``test_ring_steps_on_one_gpu_match_full_attention``'s computation of the last rank, so that ``sage_merge_states`` runs fenced: its running
    state and its output are this test's allocations (made under the fence), the partial results are ``sageattn``'s."""
    W, B, H, Lc, D = 3, 1, 4, 384 - 11, 128
    g = torch.Generator().manual_seed(21)
    q = torch.randn(B, H, Lc, D, generator=g).to(BF16)
    ks = [(torch.randn(B, H, Lc, D, generator=g) + torch.randn(1, H, 1, D, generator=g)).to(BF16) for _ in range(W)]
    vs = [torch.randn(B, H, Lc, D, generator=g).to(BF16) for _ in range(W)]
    sched = [(s, j, m) for s, j, m in ring.shard_schedule(W - 1, W, causal) if m != "skip"]
    assert len(sched) == W

    def call(qs, *kv):
        acc = torch.empty(B, H, Lc, D, dtype=torch.float32, device=DEV)
        lse = torch.empty(B, H, Lc, dtype=torch.float32, device=DEV)
        out = torch.empty_like(qs)
        for idx, (s, j, mode) in enumerate(sched):
            o_s, lse_s = sa.sageattn(qs, kv[j], kv[W + j], is_causal=(mode == "causal"), return_lse=True)
            ring.merge_states(acc, lse, o_s, lse_s, first=(idx == 0), out=out if idx == len(sched) - 1 else None)
        return out, lse, acc

    run_fenced(call, [In(q)] + [In(t) for t in ks + vs])


# ------------------------------------------------------------------------------------------------ caller-provided outputs
def _gapped_plain(shape, dtype, layout, gap):
    seq = 2 if layout == "HND" else 1
    full = list(shape)
    full[seq] += gap
    return torch.zeros(full, dtype=dtype, device=DEV).narrow(seq, 0, shape[seq])


@pytest.mark.parametrize("layout", ["HND", "NHD"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("pv,D,odt", [("f16_rows", 64, F16), ("f16_image", 128, BF16), ("f8", 64, BF16), ("f8", 128, F16)])
def test_attention_ops_write_only_the_rows_of_a_caller_s_output(pv, D, odt, causal, layout):
    """``ops.qk_int8_sv_f16_attn_impl`` / ``ops.qk_int8_sv_f8_attn_impl`` take ``o`` from the caller: a view with 8 guard rows behind every head (NHD: every batch),
    ragged Lq.  The guard rows and the guards stay intact; the owned rows are the bits of a run into a plain tensor."""
    B, Hq, Hkv, Lq, Lk = (2, 4, 2, 203, 203) if causal else (2, 4, 2, 203, 333)
    ins = qkv(B, Hq, Hkv, Lq, Lk, D, F16, seed=13 + D, layout=layout)
    code = 0 if layout == "NHD" else 1
    seq = 2 if layout == "HND" else 1

    def run(q, k, v, o):
        km = sq.channel_mean(k, layout).unsqueeze(seq)
        if pv == "f8":
            q8, qs, k8, ks = sq.per_thread_int8(q, k, km=km, tensor_layout=layout)
            v_image, v_scale, _ = sq.per_channel_fp8(v, tensor_layout=layout)
            return sa_ops.qk_int8_sv_f8_attn_impl(q8, k8, v_image, o, qs, ks, v_scale, None, code, int(causal), _cabi.GRAN_PER_THREAD, 32,
                                                  sc._sm_log2(D ** -0.5), _cabi.PV_ACCUM_TWO_LEVEL, 1)
        q8, qs, k8, ks = sq.per_block_int8(q, k, km=km, tensor_layout=layout)
        vv = v if pv == "f16_rows" else sq.prep_v_fp16(v, layout)
        return sa_ops.qk_int8_sv_f16_attn_impl(q8, k8, vv, o, qs, ks, None, code, int(causal), _cabi.GRAN_PER_BLOCK, 128, 1.0, _cabi.PV_ACCUM_TRITON, 1)

    q, k, v = (i.plain() for i in ins)
    o_want = torch.zeros(q.shape, dtype=odt, device=DEV)
    lse_want = run(q, k, v, o_want)
    o_gap = _gapped_plain(q.shape, odt, layout, 8)
    lse_gap = run(q, k, v, o_gap)
    torch.cuda.synchronize()
    assert torch.equal(o_gap, o_want) and torch.equal(lse_gap, lse_want) and bool(torch.isfinite(o_want.float()).all())
    for fill in FILLS:
        with Fence(fill) as f:
            o = f.output(q.shape, odt, gap_rows=8, tensor_layout=layout)
            lse = run(*[i.fenced(f) for i in ins], o)
            f.check()                              # the guards of every arena and the gap rows of o
            assert f.package_sites() and f.owns(lse) and f.owns(o)
            assert torch.equal(o, o_want) and torch.equal(lse, lse_want) and bool(torch.isfinite(lse).all())


@pytest.mark.parametrize("B,Hq,Hkv,Lq,Lk,D,S,causal,dtype", [
    (1, 2, 1, 333, 333, 128, 5, True, F16),
    (1, 4, 1, 130, 2048 + 77, 128, 3, False, BF16),
    (2, 2, 1, 63, 1024, 64, 2, False, F16),
])
def test_split_exact_chunk_max_writes_only_its_buffer(B, Hq, Hkv, Lq, Lk, D, S, causal, dtype):
    """``sage_split_exact_chunk_max`` through the C ABI, as test_gpu_split_exact.py calls it: the ``chunk_max`` buffer [B, Hq * S, Lq] inside an arena."""
    ins = qkv(B, Hq, Hkv, Lq, Lk, D, dtype, seed=Lq + Lk + D)[:2]
    sm_log2 = sc._sm_log2(D ** -0.5)
    dt = _cabi.DTYPE_F16 if dtype == F16 else _cabi.DTYPE_BF16

    def run(q, k, out):
        _, _, k_int8, k_scale = sq.per_thread_int8(q, k)
        _, _, _, _, q_sb, q_sh, q_sl = sq._dims(q, "HND")
        _, _, _, _, k_sb, k_sh, k_sl = sq._dims(k_int8, "HND")
        rc = _cabi.load().sage_split_exact_chunk_max(sq._p(q), sq._p(k_int8), sq._p(k_scale), sq._p(out), B, Hq, Hkv, S, Lq, Lk, D,
                                                     q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, int(causal), sm_log2, dt, sq._stream(q))
        _cabi.check(rc, "sage_split_exact_chunk_max")
        torch.cuda.synchronize()

    want = torch.full((B, Hq * S, Lq), 7.0, dtype=torch.float32, device=DEV)
    run(*[i.plain() for i in ins], want)
    assert not bool(want.isnan().any()) and not bool((want == 7.0).all())
    for fill in FILLS:
        with Fence(fill) as f:
            out = f.output((B, Hq * S, Lq), torch.float32)
            run(*[i.fenced(f) for i in ins], out)
            f.check()
            assert torch.equal(out, want), "every element of chunk_max is written, with the bits of the plain run"


@pytest.mark.parametrize("dtype,layout,D,L", [(F16, "HND", 128, 333), (BF16, "NHD", 64, 130), (BF16, "HND", 96, 17)])
def test_merge_states_writes_only_the_rows_of_a_caller_s_output(dtype, layout, D, L):
    """``sage_merge_states`` as test_merge_states_matches_formula calls it (-inf rows included): the running state inside arenas, ``out`` a view
    with 8 guard rows behind every head (NHD: every batch)."""
    g = torch.Generator().manual_seed(12)
    B, H = 2, 3
    oa, ob = torch.randn(B, H, L, D, generator=g).to(dtype), torch.randn(B, H, L, D, generator=g).to(dtype)
    la, lb = 4.0 * torch.randn(B, H, L, generator=g), 4.0 * torch.randn(B, H, L, generator=g)
    lb[0, 0, :5] = float("-inf")
    la[1, 2, 3] = float("-inf")
    la[1, 1, 7] = lb[1, 1, 7] = float("-inf")
    if layout == "NHD":
        oa, ob = oa.transpose(1, 2).contiguous(), ob.transpose(1, 2).contiguous()
    ins = [In(oa), In(la), In(ob), In(lb)]

    def run(oa, la, ob, lb, acc, lse, out):
        ring.merge_states(acc, lse, oa, la, layout, first=True)
        ring.merge_states(acc, lse, ob, lb, layout, out=out)
        torch.cuda.synchronize()

    acc_w, lse_w = torch.zeros(B, H, L, D, device=DEV), torch.zeros(B, H, L, device=DEV)
    out_w = torch.zeros(oa.shape, dtype=dtype, device=DEV)
    run(*[i.plain() for i in ins], acc_w, lse_w, out_w)
    for fill in FILLS:
        with Fence(fill) as f:
            acc, lse = f.output((B, H, L, D), torch.float32), f.output((B, H, L), torch.float32)
            out = f.output(oa.shape, dtype, gap_rows=8, tensor_layout=layout)
            run(*[i.fenced(f) for i in ins], acc, lse, out)
            f.check()
            assert torch.equal(acc, acc_w) and torch.equal(lse, lse_w) and torch.equal(out, out_w)
            assert bool(torch.isfinite(acc).all()) and bool(torch.isfinite(out.float()).all())


# ------------------------------------------------------------------------------------------------ the route list
ROUTES = {p.values[0] for p in DENSE} | {p.values[0] for p in VARLEN}        # the public names that have fenced cases


def test_every_public_entry_point_has_fenced_cases():
    """Every public name of the package that launches a kernel has cases above: a new entry point without a fenced case fails here."""
    public = {n for n in sa.__all__ if callable(getattr(sa, n))}
    assert public == ROUTES, f"public names without fenced cases: {sorted(public - ROUTES)}; stale entries: {sorted(ROUTES - public)}"
    ids = [p.id for p in DENSE] + [p.id for p in VARLEN] + [p.id for p in MASKED]
    assert len(ids) == len(set(ids)), sorted(i for i in set(ids) if ids.count(i) > 1)
