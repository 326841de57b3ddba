"""GPU: the wide FP8-PV entries inside guarded, poisoned memory (tests/fence.py): ``hd256.sageattn_hd256``, ``qk192.sageattn_qk192``,
``qk192_varlen.sageattn_qk192_varlen`` and ``mla_decode.sageattn_mla_decode`` with ``mla_quantize_latent``.

tests/test_gpu_fence.py finds its routes through ``sageattention_amd.__all__``, which these entries are deliberately not in; this file is
its pattern (``run_fenced`` and ``In`` are imported from it) pointed at them.  A call runs plainly, then under each fill of ``FILLS`` with
its inputs placed by the fence and every allocation of the package -- K and V images, scales, means, workspaces, ``o``, ``lse`` -- between
two guards and poisoned: results bit-identical to the plain run, every guard byte intact, ``package_sites()`` non-empty, the returned ``o``
inside an arena.  The LSE is finite except where the contract says ``-inf`` (a row in front of key 0, a sequence or sample without keys):
there it is exactly ``-inf`` and ``o`` exactly ``+0``.  No tolerance appears anywhere.

The guard.  tests/fence.py's default of 64 KiB covers two stages of the D <= 128 kernels (48 KiB).  The tiles of this family are larger:
a 64-key K tile is 64 x 256 = 16384 bytes (hd256), 64 x 192 = 12288 (qk192 and its packed form) and 64 x 576 = 36864 for the MLA kernel
(include/sage_mla_gfx950.h: ``K image [B, ntile, 36864]``), an e4m3 V tile 16384, 8192 and 64 x 512 = 32768 (``V image [B, ntile,
32768]``).  Every loop of the family keeps a two-slot ring per operand and requests tile t + 1 at the top of tile t: a prefetch distance
of one tile, two tiles of each operand in flight.  A stray access anywhere within that distance of a buffer's edge -- two stages of the
largest tile pair, 2 x (36864 + 32768) = 139264 bytes = 136 KiB, already a multiple of 128 -- lands inside ``WIDE_GUARD``.

Each case is the smallest shape that reaches the mechanism it is named for (tests/test_gpu_hd256.py and its siblings name them): a partial
wave with a ragged second tile (33, 65), a second query block with the ring wrapping (129, 192), steady state with a ragged tail
(257, 449).  With ``gap`` the caller's q, k and v are views with guard rows behind every head (NHD: every batch), so no operand is
contiguous.  What torch allocates itself (``F.pad`` at D 136, 160 / 72) is not fenced; the package's own allocations behind it are.
"""
import math

import pytest
import torch

import test_gpu_fence as base
from fence import FILLS, Fence
from test_gpu_fence import In, run_fenced
from test_gpu_qk192_varlen import CASES as VARLEN_FEATURE_CASES, _inputs as varlen_inputs

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
WIDE_GUARD = (2 * (36864 + 32768) + 127) // 128 * 128
MODULES = ("hd256", "qk192", "qk192_varlen", "mla_decode")


class WideFence(Fence):
    """The fence ``run_fenced`` builds in this file: ``Fence(fill, guard=WIDE_GUARD)``."""
    made = 0

    def __init__(self, fill):
        super().__init__(fill, guard=WIDE_GUARD)
        WideFence.made += 1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def _wide_guard(monkeypatch):
    monkeypatch.setattr(base, "Fence", WideFence)


def _run(entry, call, inputs, lse_neg_inf_ok=False):
    before = WideFence.made
    seen = run_fenced(call, inputs, lse_neg_inf_ok=lse_neg_inf_ok)
    assert WideFence.made == before + len(FILLS) and WIDE_GUARD == 139264, "run_fenced did not build this file's fences"
    print(f"FENCE {entry}: allocations {sorted({(fn, str(dt).replace('torch.', '')) for fn, _, dt in seen.allocs})} at {sorted(seen.sites)}")
    return seen


def _contract(o_rows, lse_rows, empty, what):
    """``o_rows`` ``[R, ...]`` and ``lse_rows`` ``[R, ...]`` by query row; ``empty`` bool ``[R]``: the rows that see no key."""
    empty = empty.to(lse_rows.device)
    assert bool((lse_rows[empty] == -math.inf).all()) and bool(torch.isfinite(lse_rows[~empty]).all()), f"{what}: lse is -inf exactly in the rows without a key"
    blind = o_rows[empty].float()
    assert bool((blind == 0).all()) and not bool(torch.signbit(blind).any()), f"{what}: o is +0 in the rows without a key"


def _qkv(Lq, Lk, Dqk, Dv, dtype, layout, gap, seed, B=2, Hq=4, Hkv=2):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Hq, Lq, Dqk, generator=g).to(dtype)
    k = (torch.randn(B, Hkv, Lk, Dqk, generator=g) + torch.randn(1, Hkv, 1, Dqk, generator=g)).to(dtype)
    v = torch.randn(B, Hkv, Lk, Dv, generator=g).to(dtype)
    if layout == "NHD":
        q, k, v = (t.transpose(1, 2).contiguous() for t in (q, k, v))
    return [In(t, gap, layout) for t in (q, k, v)]


SHAPES = ((33, 65), (129, 192), (257, 449))
CASES = {name: [] for name in ("sageattn_hd256", "sageattn_qk192", "sageattn_qk192_varlen", "sageattn_mla_decode")}

# ------------------------------------------------------------------------------------------------ sageattn_hd256, sageattn_qk192
for name, dqk, dv, small in (("sageattn_hd256", 256, 256, (136, 136)), ("sageattn_qk192", 192, 128, (160, 72))):
    n = 0
    for layout in ("HND", "NHD"):
        for causal in (False, True):
            for Lq, Lk in SHAPES:                    # read in place: the package pads nothing
                dtype, n = (F16, BF16)[n % 2], n + 1
                CASES[name].append(pytest.param(Lq, Lk, dqk, dv, dtype, layout, causal, 0,
                                                id=f"{'c' if causal else 'nc'}-q{Lq}l{Lk}-d{dqk}v{dv}-{'f16' if dtype == F16 else 'bf16'}-{layout}"))
    # guard rows behind every head (HND) / every batch (NHD): no operand is contiguous; the package's own allocations behind F.pad
    CASES[name] += [pytest.param(129, 192, dqk, dv, F16, "HND", True, 8, id=f"c-q129l192-d{dqk}v{dv}-f16-HND-gap8"),
                    pytest.param(257, 449, dqk, dv, BF16, "NHD", False, 8, id=f"nc-q257l449-d{dqk}v{dv}-bf16-NHD-gap8"),
                    pytest.param(33, 65, *small, BF16, "HND", True, 0, id=f"c-q33l65-d{small[0]}v{small[1]}-bf16-HND-padded"),
                    pytest.param(129, 192, *small, F16, "NHD", False, 0, id=f"nc-q129l192-d{small[0]}v{small[1]}-f16-NHD-padded")]


@pytest.mark.parametrize("Lq,Lk,D,Dv,dtype,layout,causal,gap", CASES["sageattn_hd256"])
def test_hd256_inside_the_fence(Lq, Lk, D, Dv, dtype, layout, causal, gap):
    from sageattention_amd.hd256 import sageattn_hd256
    ins = _qkv(Lq, Lk, D, Dv, dtype, layout, gap, seed=Lq + 3 * Lk + D)
    seen = _run("sageattn_hd256", lambda q, k, v: sageattn_hd256(q, k, v, tensor_layout=layout, is_causal=causal, return_lse=True), ins)
    assert "sageattn_hd256" in seen.funcs, sorted(seen.funcs)
    assert any(dt == torch.uint8 and shape[-1] == 64 * 256 for _, shape, dt in seen.allocs), "the K and V images were not allocated under the fence"


@pytest.mark.parametrize("Lq,Lk,Dqk,Dv,dtype,layout,causal,gap", CASES["sageattn_qk192"])
def test_qk192_inside_the_fence(Lq, Lk, Dqk, Dv, dtype, layout, causal, gap):
    from sageattention_amd.qk192 import sageattn_qk192
    ins = _qkv(Lq, Lk, Dqk, Dv, dtype, layout, gap, seed=Lq + 3 * Lk + Dqk)
    seen = _run("sageattn_qk192", lambda q, k, v: sageattn_qk192(q, k, v, tensor_layout=layout, is_causal=causal, return_lse=True), ins)
    assert "sageattn_qk192" in seen.funcs, sorted(seen.funcs)


# ------------------------------------------------------------------------------------------------ sageattn_qk192_varlen
VARLEN_KW = {"none": dict(is_causal=False, causal_align="top_left"), "top_left": dict(is_causal=True, causal_align="top_left"),
             "bottom_right": dict(is_causal=True, causal_align="bottom_right")}
for case in VARLEN_FEATURE_CASES[1:4]:
    for mask in VARLEN_KW:
        CASES["sageattn_qk192_varlen"].append(pytest.param(case, mask, id="-".join(f"{a}x{b}" for a, b in case[0]) + "-" + mask))


@pytest.mark.parametrize("case,mask", CASES["sageattn_qk192_varlen"])
def test_qk192_varlen_inside_the_fence(case, mask):
    """The packed q, k and v are placed with ``f.input``: the rows in front of sequence 0 and behind the last sequence are guard bytes.
    Rows without a key -- a sequence without keys; bottom-right, the first ``Lq_s - Lk_s`` rows -- are ``+0`` / ``-inf`` exactly."""
    from sageattention_amd.qk192_varlen import sageattn_qk192_varlen
    seqs, Dqk, Dv, heads, dtype, smooth_k, sm_scale = case
    q, k, v, cu_q, cu_k = varlen_inputs(seqs, Dqk, Dv, heads, dtype)
    mq, mk = max(a for a, _ in seqs), max(b for _, b in seqs)
    empty = torch.cat([torch.arange(lq) < (lq if lk == 0 else (max(lq - lk, 0) if mask == "bottom_right" else 0)) for lq, lk in seqs])

    def call(q, k, v, cu_q, cu_k):
        o, lse = sageattn_qk192_varlen(q, k, v, cu_q, cu_k, mq, mk, sm_scale=sm_scale, smooth_k=smooth_k, return_lse=True, **VARLEN_KW[mask])
        _contract(o, lse.t(), empty, f"qk192_varlen {mask}")
        return o, lse

    seen = _run("sageattn_qk192_varlen", call, [In(t) for t in (q, k, v, cu_q, cu_k)], lse_neg_inf_ok=bool(empty.any()))
    assert "sageattn_qk192_varlen" in seen.funcs, sorted(seen.funcs)


# ------------------------------------------------------------------------------------------------ sageattn_mla_decode
class PoisonedKV(In):
    """The latent cache with the rows from ``kv_lens[b]`` on poisoned: random in the plain run, the fence's fill under it (NaN under 0xFF,
    finite under 0x5A), written before the call.  The result must not differ between the three."""

    def __init__(self, t, lens):
        super().__init__(t)
        self.lens = lens

    def fenced(self, f):
        dst = f.input(self.t)
        for b, n in enumerate(self.lens):
            dst[b, n:].view(torch.uint8).fill_(f.fill)
        if f.fill == 0xFF:
            assert all(bool(dst[b, n:].isnan().all()) for b, n in enumerate(self.lens))
        return dst


class StridedQ(In):
    """q as a view of a larger tensor, as ``test_quantise_once_and_strided_q`` builds it, the larger tensor inside an arena: every stride
    differs from the contiguous one, and what lies between q's rows is the fill."""

    def _view(self, big):
        Lq, Hq = self.t.shape[1:3]
        view = big[:, :Lq, 8:, 64:]
        view.copy_(self.t)
        return view

    def _shape(self):
        B, Lq, Hq, _ = self.t.shape
        return (B, Lq + 1, Hq + 8, 640)

    def plain(self):
        return self._view(torch.zeros(self._shape(), dtype=self.t.dtype, device=base.DEV))

    def fenced(self, f):
        return self._view(f.output(self._shape(), self.t.dtype))


# (Lq, Hq, kv_lens, Lk): tests/test_gpu_mla_decode.py names the mechanism of each
MLA_SHAPES = ((1, 16, [65, 33], 65), (2, 128, [449, 257], 449), (3, 48, [200, 70], 200), (4, 16, [2, 0], 64))
for i, (Lq, Hq, lens, Lk) in enumerate(MLA_SHAPES):
    for mode in ("kv", "latent", "strided_q"):
        CASES["sageattn_mla_decode"].append(pytest.param(Lq, Hq, lens, Lk, (BF16, F16)[i % 2], mode, id=f"q{Lq}h{Hq}-{'_'.join(map(str, lens))}-{mode}"))


@pytest.mark.parametrize("Lq,Hq,lens,Lk,dtype,mode", CASES["sageattn_mla_decode"])
def test_mla_decode_inside_the_fence(Lq, Hq, lens, Lk, dtype, mode):
    """``kv``: the call quantises the latent itself.  ``latent``: ``mla_quantize_latent`` runs fenced as well and its images serve two
    attention calls.  ``strided_q``: q is a view inside a poisoned arena.  A position in front of key 0 and a sample without keys give
    ``+0`` / ``-inf`` exactly; the rows of ``kv`` behind a sample's length are poison and are never read."""
    from sageattention_amd.mla_decode import mla_quantize_latent, sageattn_mla_decode
    g = torch.Generator().manual_seed(1000 * Lq + Hq + Lk)
    q = torch.randn(2, Lq, Hq, 576, generator=g).to(dtype)
    kv = (torch.randn(2, Lk, 576, generator=g) + torch.randn(1, 1, 576, generator=g)).to(dtype)
    empty = torch.tensor([[n - Lq + i < 0 for i in range(Lq)] for n in lens])                   # [B, Lq]

    def call(q, kv, kv_lens):
        if mode == "latent":
            lat = mla_quantize_latent(kv, kv_lens)
            outs = sageattn_mla_decode(q, lat, return_lse=True) + sageattn_mla_decode(q, lat, return_lse=True)
            assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]), "the second call on the same images differs"
        else:
            outs = sageattn_mla_decode(q, kv, kv_lens, return_lse=True)
        _contract(outs[0].flatten(0, 1), outs[1].transpose(1, 2).flatten(0, 1), empty.flatten(), f"mla_decode {mode}")
        return outs

    ins = [StridedQ(q) if mode == "strided_q" else In(q), PoisonedKV(kv, lens), In(torch.tensor(lens, dtype=torch.int32))]
    seen = _run("sageattn_mla_decode", call, ins, lse_neg_inf_ok=bool(empty.any()))
    assert {"mla_quantize_latent", "sageattn_mla_decode"} <= seen.funcs, sorted(seen.funcs)


# ------------------------------------------------------------------------------------------------ the entry list
def test_every_wide_entry_point_has_fenced_cases():
    """The entries with fenced cases above are the callables named ``sageattn_*`` that the four modules define: a fifth wide entry added
    later fails here instead of going unfenced."""
    import importlib
    found = set()
    for m in MODULES:
        mod = importlib.import_module(f"sageattention_amd.{m}")
        found |= {n for n, f in vars(mod).items() if n.startswith("sageattn_") and callable(f) and getattr(f, "__module__", None) == mod.__name__}
    fenced = {name for name, cases in CASES.items() if cases}
    assert fenced == found, f"wide entries without fenced cases: {sorted(found - fenced)}; stale entries: {sorted(fenced - found)}"
    ids = [p.id for cases in CASES.values() for p in cases]
    assert len(ids) == len(set(ids)), sorted(i for i in set(ids) if ids.count(i) > 1)
