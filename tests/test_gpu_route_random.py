"""GPU: a seeded random sweep of the keyword family of the dense FP8-PV entry point -- ``kv_lens``, ``q_start`` / ``causal_align``,
``window_size``, ``pack_gqa`` -- in the manner of test_gpu_parity.py::test_random_shapes_vs_oracle (``SAGE_RANDOM_SEEDS`` seeds, default 100).

The feature tests and the tile-count sweeps walk chosen tables; a hazard that lives in one instantiation at one tile count beside one
combination of keywords is what a seeded sweep found before.  ``loop_plan.random_call`` draws the call (pure Python:
tests/test_loop_plan_host.py checks on the CPU that at least 95 of the first 100 seeds have a sample in which half the rows see a key).

Reference: ``ref_window.attn_window`` under ``ref_window.visible_from_keywords`` -- the predicate from the PUBLIC keywords -- on the oracle's
quantised operands of the sample's valid keys, at test_gpu_window.py::_check's bar (``2e-3 max|ref| + 2 output ulps``, LSE within 5e-3, rows
without keys exactly +0 / -inf and the predicate's rows).  A drawn ``pack_gqa=True`` call also equals its unpacked twin bit for bit.
Reference cost on the CPU, measured over the first 30 seeds: 0.05 s per seed on average, 0.16 s at the most.
"""
import os

import pytest
import torch

import loop_plan as lp
import ref_window as rw
from test_gpu_route_tile_counts import check_sample

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi
    DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("SAGE_RANDOM_SEEDS", "100")))))
def test_random_keyword_calls_vs_restatement(oracle_mod, seed):
    c = lp.random_call(seed)
    B, Hkv, Hq, Lq, Lk, D, layout, smooth_k = c["B"], c["Hkv"], c["Hkv"] * c["group"], c["Lq"], c["Lk"], c["D"], c["layout"], c["smooth_k"]
    dt = torch.float16 if c["dtype"] == "f16" else torch.bfloat16
    code = 0 if c["dtype"] == "f16" else 1
    g = torch.Generator().manual_seed(77000 + seed)
    q = torch.randn(B, Hq, Lq, D, generator=g).to(dt).to(DEV)
    k = (torch.randn(B, Hkv, Lk, D, generator=g) + torch.randn(1, Hkv, 1, D, generator=g)).to(dt).to(DEV)      # (padding rows: random data)
    v = torch.randn(B, Hkv, Lk, D, generator=g).to(dt).to(DEV)
    lay = (lambda t: t) if layout == "HND" else (lambda t: t.transpose(1, 2).contiguous())
    hnd = (lambda t: t) if layout == "HND" else (lambda t: t.transpose(1, 2))
    ints = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    kw = dict(tensor_layout=layout, is_causal=c["is_causal"], smooth_k=smooth_k, return_lse=True, kv_lens=ints(c["lens"]))
    if c["window_size"] is not None:
        kw["window_size"] = c["window_size"]
    if c["causal_align"] != "top_left":
        kw["causal_align"] = c["causal_align"]
    if c["q_start"] is not None:
        kw["q_start"] = c["q_start"] if isinstance(c["q_start"], int) else ints(c["q_start"])
    desc = f"seed {seed}: " + " ".join(f"{a}={c[a]}" for a in ("D", "dtype", "layout", "smooth_k", "B", "Hkv", "group", "Lq", "Lk", "lens", "is_causal",
                                                             "causal_align", "q_start", "window_size", "pack_gqa"))
    print(desc)
    o, lse = sa.sageattn_qk_int8_pv_fp8_cuda(lay(q), lay(k), lay(v), pack_gqa=True if c["pack_gqa"] else None, **kw)
    assert o.shape == lay(q).shape and o.dtype == dt and lse.shape == (B, Hq, Lq), desc
    if c["pack_gqa"]:
        o2, lse2 = sa.sageattn_qk_int8_pv_fp8_cuda(lay(q), lay(k), lay(v), pack_gqa=False, **kw)
        assert torch.equal(o, o2), f"{desc}: packed o differs from the unpacked call in {int((o != o2).sum())} elements"
        assert torch.equal(lse, lse2), f"{desc}: packed lse differs from the unpacked call in {int((lse != lse2).sum())} rows"
    o = hnd(o)
    for b, (n, s, ws, causal) in enumerate(lp.random_call_geometry(c)):
        keep = rw.visible_from_keywords(Lq, Lk, ws, causal, s, n)[:, :n]
        check_sample(oracle_mod, f"seed {seed} sample {b} (len {n}, offset {s}, window {ws})", q[b:b + 1], k[b:b + 1, :, :n].contiguous(),
                     v[b:b + 1, :, :n].contiguous(), code, D, smooth_k, keep, o[b:b + 1], lse[b:b + 1])
