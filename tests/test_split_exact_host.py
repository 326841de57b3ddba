"""CPU: the exact split-KV route's interface -- keyword errors before any GPU work, the plan, the torch.compile refusal, the C-ABI argument
checks of its three entries, and the resources of its kernels (zero scratch, the family's occupancy; the MFMA hazard lint)."""
import ctypes
import os

import pytest
import torch

import util  # noqa: F401  (sys.path)
from sageattention_amd import _cabi, core as sc

HIPCC = "/opt/rocm/bin/hipcc"


def _cpu_qkv(Lk=256, D=64):
    return torch.zeros(1, 2, 16, D, dtype=torch.float16), torch.zeros(1, 2, Lk, D, dtype=torch.float16), torch.zeros(1, 2, Lk, D, dtype=torch.float16)


@pytest.mark.parametrize("kw,msg", [
    (dict(fp8_scores="folded"), "exact score form"),
    (dict(qk_quant_gran="per_warp"), "per_thread"),
    (dict(qk_quant_gran="per_block"), "per_thread"),
    (dict(pv_accum_dtype="fp32"), "two-level"),
    (dict(fuse_q_quant=False), "fused Q"),
    (dict(split_kv=3), "divide"),                      # 4 whole tiles
    (dict(split_kv=1), "divide"),
    (dict(split_kv="half"), "'auto'"),
])
def test_keyword_errors_come_before_any_gpu_work(kw, msg):
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match=msg):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, split_kv_exact=True, **kw)


def test_flag_off_changes_nothing_and_ragged_counts_whole_tiles():
    q, k, v = _cpu_qkv(Lk=256 + 13)
    with pytest.raises(AssertionError, match="cuda"):        # (no route override: the ordinary input check of a CPU tensor)
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, split_kv_exact=False, split_kv=3, pv_accum_dtype="fp32")
    with pytest.raises(AssertionError, match="cuda"):        # S = 2 divides the 4 whole tiles of 269 keys: accepted, then the input check
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, split_kv_exact=True, split_kv=2)


def test_plan():
    assert sc._split_exact_plan(1, 32, 128, 32768, False, None) == sc._split_kv_plan(1, 32, 128, 32768, False, "auto") >= 2
    assert sc._split_exact_plan(1, 32, 128, 32768 + 77, False, None) == sc._split_kv_plan(1, 32, 128, 32768 + 64, False, "auto") == 9
    assert sc._split_exact_plan(2, 32, 8192, 8192, False, None) == 0
    assert sc._split_exact_plan(1, 32, 128, 32768, True, "auto") == 0
    assert sc._split_exact_plan(1, 2, 384, 384, True, 2) == 2
    assert sc._split_exact_plan(1, 2, 960, 960 + 5, True, 5) == 5
    assert sc._split_exact_plan(1, 32, 128, 32768, False, 0) == 0
    with pytest.raises(ValueError):
        sc._split_exact_plan(1, 2, 960, 960, False, 4)        # 15 tiles
    with pytest.raises(ValueError):
        sc._split_exact_plan(1, 2, 960, 960, False, True)
    with pytest.raises(ValueError, match="divide"):           # fewer than 64 keys: no whole tile to split
        sc._split_exact_plan(1, 2, 16, 40, False, 2)


def test_torch_compile_refuses_a_truthy_flag_only():
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match="split_kv_exact: route overrides"):
        sc._compiled_call("fp8", q, k, v, "HND", False, "per_thread", None, "fp32+fp32", True, False, False, {"split_kv_exact": True})
    called = []
    orig = sc.ops.sageattn_call
    try:
        sc.ops.sageattn_call = lambda *a, **kw: called.append(a) or (q, None)
        sc._compiled_call("fp8", q, k, v, "HND", False, "per_thread", None, "fp32+fp32", True, False, False, {"split_kv_exact": False})
    finally:
        sc.ops.sageattn_call = orig
    assert len(called) == 1


def test_abi_entries_reject_bad_arguments_without_a_gpu():
    lib = _cabi.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15

    # pass 1: (q, k, k_scale, out, B, Hq, Hkv, S, Lq, Lk, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, causal, sm, q_dtype, stream)
    def cm(**o):
        return lib.sage_split_exact_chunk_max(o.get("q", p), p, p, o.get("out", p), 1, o.get("Hq", 2), 2, o.get("S", 2), 16, o.get("Lk", 256),
                                              o.get("D", 64), 0, 0, o.get("q_sl", 64), 0, 0, 64, 0, 1.0, o.get("qdt", 0), None)
    for kw, msg in ((dict(D=96), b"head_dim"), (dict(q=p + 2), b"aligned"), (dict(Hq=3), b"divisible"), (dict(S=3), b"kv_split"),
                    (dict(S=8), b"kv_split"), (dict(Lk=0), b"empty"), (dict(qdt=5), b"q_dtype"), (dict(q_sl=60), b"q strides"),
                    (dict(out=None), b"chunk_max")):
        assert cm(**kw) == -1 and msg in lib.sage_last_error(), (kw, lib.sage_last_error())

    # pass 2: (q, k, v_image, o_part, lse_part, k_scale, v_scale, v_mean, chunk_max, B, Hq, Hkv, S, tail, Lq, Lk, D, strides x6,
    #          causal, sm, q_dtype, stream, attr)
    def p2(**o):
        return lib.sage_attn_fused_q_pv_f8_split_exact(p, p, p, o.get("o", p), p, p, o.get("vs", p), None, o.get("cm", p), 1, 2, 2,
                                                       o.get("S", 2), o.get("tail", 0), 16, o.get("Lk", 256), o.get("D", 64),
                                                       0, 0, 64, 0, 0, 64, 0, 1.0, 0, None, o.get("attr", None))
    for kw, msg in ((dict(D=96), b"head_dim"), (dict(S=3), b"kv_split"), (dict(vs=None), b"null"), (dict(cm=None), b"null"),
                    (dict(tail=2), b"tail"), (dict(tail=1), b"ragged"), (dict(o=p + 4), b"aligned")):
        assert p2(**kw) == -1 and msg in lib.sage_last_error(), (kw, lib.sage_last_error())
    folded = _cabi.launch_attr(None, folded_scores=True)
    assert p2(attr=_cabi.attr_arg(folded)) == -1 and b"exact score form" in lib.sage_last_error()

    # the FP32 merge: (o_part, lse_part, o_tail, lse_tail, o_out, lse_out, B, S, H, group, L, D, o strides, dtype, stream)
    def mg(**o):
        return lib.sage_merge_split_f32(p, p, o.get("ot", None), o.get("lt", None), o.get("oo", p), None, 1, 2, o.get("H", 4), 2, 16,
                                        o.get("D", 64), 0, 0, 64, o.get("dt", 0), None)
    for kw, msg in ((dict(D=12), b"multiple of 8"), (dict(H=3), b"divisible"), (dict(ot=p), b"together"), (dict(oo=None), b"null"),
                    (dict(dt=4), b"out_dtype"), (dict(oo=p + 2), b"aligned")):
        assert mg(**kw) == -1 and msg in lib.sage_last_error(), (kw, lib.sage_last_error())


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_exact_split_units_do_not_spill():
    """sage_attn_d{128,64}_f8s.hip: causal x fp16 / bf16 q seeded kernels at the family's occupancy (D = 128: 2, D = 64: 3 waves / SIMD);
    sage_split_exact.hip: pass 1, no scratch."""
    import test_build_resources as tbr
    from concurrent.futures import ThreadPoolExecutor
    units = ("sage_attn_d128_f8s.hip", "sage_attn_d64_f8s.hip", "sage_split_exact.hip")
    with ThreadPoolExecutor(max_workers=3) as ex:
        reports = dict(zip(units, ex.map(tbr._resource_report, units)))
    for unit in units[:2]:
        mine = {k: v for k, v in reports[unit].items() if "sage_attn_kernel" in k}
        assert len(mine) == 4, (unit, sorted(mine))
        for name, res in mine.items():
            assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0, (unit, name, res)
            assert res["Occupancy"] >= (2 if "128" in unit else 3), (unit, name, res)
    cm = {k: v for k, v in reports["sage_split_exact.hip"].items() if "chunk_max_kernel" in k}
    assert len(cm) == 8, sorted(cm)
    for name, res in cm.items():
        assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0, (name, res)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_exact_split_units_pass_the_hazard_lint():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import mfma_hazard_lint as lint
    for unit in ("sage_attn_d128_f8s.hip", "sage_attn_d64_f8s.hip"):
        assert unit in lint.UNITS
        findings, n_mfma = lint.lint(lint.listing(unit))
        assert n_mfma >= 200 and not findings, (unit, n_mfma, findings[:5])
