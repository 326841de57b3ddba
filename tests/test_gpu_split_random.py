"""GPU: a seeded random sweep of ``num_splits=`` on the dense FP8-PV entry point, in the manner of test_gpu_route_random.py (``SAGE_RANDOM_SEEDS``
seeds, default 100).

``loop_plan.random_split_call`` draws the call with a random stream of its own -- head size, dtype, layout, smooth_k, B, heads and group (5 among
them: a packed workgroup with idle waves), one query block of rows, the padded key length (up to 2560), per-sample lengths, one kind of
offset (none non-causal, top-left, bottom_right, an int, a tensor), the chunk count (2, 3, 4, 7, one tile per chunk, three chunks past the tensor,
255) and ``pack_gqa`` where the route takes it.  tests/test_loop_plan_host.py checks on the CPU that at least 95 of the first 100 seeds have a sample
in which half the rows see a key and that every chunk count and offset kind is drawn.

Three checks per seed:
  * every sample against ``ref_window.attn_window`` under ``ref_window.visible_from_keywords`` on the oracle's quantised operands of its valid
    keys, at test_gpu_route_tile_counts.py::check_sample's bar (2e-3 max|ref| + 2 output ulps, LSE within 5e-3, rows without keys +0 / -inf);
  * the call against its twin without ``num_splits`` at test_gpu_kv_split.py::_distance's bars for "summation order only";
  * a drawn ``pack_gqa=True`` call equals its unpacked split twin bit for bit.
"""
import os

import pytest
import torch

import loop_plan as lp
import ref_window as rw
from test_gpu_kv_split import _distance
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
def test_random_split_calls(oracle_mod, seed):
    c = lp.random_split_call(seed)
    B, Hkv, Hq, Lq, Lk, D, layout, smooth_k, S = c["B"], c["Hkv"], c["Hkv"] * c["group"], c["Lq"], c["Lk"], c["D"], c["layout"], c["smooth_k"], c["S"]
    dt = torch.float16 if c["dtype"] == "f16" else torch.bfloat16
    code = 0 if c["dtype"] == "f16" else 1
    g = torch.Generator().manual_seed(79000 + seed)
    q = torch.randn(B, Hq, Lq, D, generator=g).to(dt).to(DEV)
    k = (torch.randn(B, Hkv, Lk, D, generator=g) + torch.randn(1, Hkv, 1, D, generator=g)).to(dt).to(DEV)      # (padding rows: random data)
    v = torch.randn(B, Hkv, Lk, D, generator=g).to(dt).to(DEV)
    lay = (lambda t: t) if layout == "HND" else (lambda t: t.transpose(1, 2).contiguous())
    hnd = (lambda t: t) if layout == "HND" else (lambda t: t.transpose(1, 2))
    ints = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    kw = dict(tensor_layout=layout, is_causal=c["is_causal"], smooth_k=smooth_k, return_lse=True, kv_lens=ints(c["lens"]))
    if c["causal_align"] != "top_left":
        kw["causal_align"] = c["causal_align"]
    if c["q_start"] is not None:
        kw["q_start"] = c["q_start"] if isinstance(c["q_start"], int) else ints(c["q_start"])
    desc = f"seed {seed}: " + " ".join(f"{a}={c[a]}" for a in ("D", "dtype", "layout", "smooth_k", "B", "Hkv", "group", "Lq", "Lk", "lens", "offset",
                                                             "q_start", "S_kind", "S", "pack_gqa"))
    print(desc)
    pack = True if c["pack_gqa"] else None
    o, lse = sa.sageattn_qk_int8_pv_fp8_cuda(lay(q), lay(k), lay(v), pack_gqa=pack, num_splits=S, **kw)
    assert o.shape == lay(q).shape and o.dtype == dt and lse.shape == (B, Hq, Lq), desc
    want = sa.sageattn_qk_int8_pv_fp8_cuda(lay(q), lay(k), lay(v), pack_gqa=pack, **kw)
    elem, rms, dl = _distance((o, lse), want, dt)
    print(f"WORST seed {seed}: element {elem:.3f} rel-RMS {rms:.3f} lse {dl:.3f} of their bars (against the call without num_splits)")
    assert elem <= 1.0 and rms <= 1.0 and dl <= 1.0, (desc, elem, rms, dl)
    if c["pack_gqa"]:
        o2, lse2 = sa.sageattn_qk_int8_pv_fp8_cuda(lay(q), lay(k), lay(v), pack_gqa=False, num_splits=S, **kw)
        assert torch.equal(o, o2), f"{desc}: packed o differs from the unpacked split in {int((o != o2).sum())} elements"
        assert torch.equal(lse, lse2), f"{desc}: packed lse differs from the unpacked split in {int((lse != lse2).sum())} rows"
    o = hnd(o)
    for b, (n, s, ws, causal) in enumerate(lp.random_call_geometry(c)):
        keep = rw.visible_from_keywords(Lq, Lk, ws, causal, s, n)[:, :n]
        check_sample(oracle_mod, f"seed {seed} sample {b} (len {n}, offset {s}, S {S})", q[b:b + 1], k[b:b + 1, :, :n].contiguous(),
                     v[b:b + 1, :, :n].contiguous(), code, D, smooth_k, keep, o[b:b + 1], lse[b:b + 1])
