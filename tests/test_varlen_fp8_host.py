"""CPU: sageattn_qk_int8_pv_fp8_varlen's interface and its C ABI entries (ABI 22) -- signature, argument errors raised before any GPU
work, and the instantiation units of its kernels (compiled for gfx950 here: no spill, the occupancy of the other attention units)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import util  # noqa: F401  (sys.path)
import sageattention
import sageattention_amd as sa
from sageattention_amd import _cabi


def test_signature_and_defaults():
    assert "sageattn_qk_int8_pv_fp8_varlen" in sa.__all__ and "sageattn_qk_int8_pv_fp8_varlen" in sageattention.__all__
    assert sageattention.sageattn_qk_int8_pv_fp8_varlen is sa.sageattn_qk_int8_pv_fp8_varlen
    sig = inspect.signature(sa.sageattn_qk_int8_pv_fp8_varlen)
    names = list(sig.parameters)
    assert names == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "is_causal", "sm_scale", "smooth_k",
                     "pv_accum_dtype", "return_lse", "kwargs"]
    d = {n: p.default for n, p in sig.parameters.items()}
    assert d["is_causal"] is False and d["sm_scale"] is None and d["smooth_k"] is True
    assert d["pv_accum_dtype"] == "fp32+fp32" and d["return_lse"] is False
    assert sig.parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD


def _packed(dev="cpu"):
    q = torch.randn(10, 4, 64, dtype=torch.float16, device=dev)
    k = torch.randn(10, 2, 64, dtype=torch.float16, device=dev)
    cu = torch.tensor([0, 3, 10], dtype=torch.int32, device=dev)
    return q, k, k.clone(), cu


@pytest.mark.parametrize("accum", ["fp32+fp16", "fp16", "fp16+fp32", "int8"])
def test_bad_pv_accum_dtype_raises_value_error(accum):
    q, k, v, cu = _packed()
    with pytest.raises(ValueError, match=re.escape(f"Unsupported pv_accum_dtype: {accum}")):
        sa.sageattn_qk_int8_pv_fp8_varlen(q, k, v, cu, cu, 7, 7, pv_accum_dtype=accum)


def test_cpu_tensors_are_rejected():
    q, k, v, cu = _packed()
    with pytest.raises(AssertionError, match="cuda"):
        sa.sageattn_qk_int8_pv_fp8_varlen(q, k, v, cu, cu, 7, 7)


def test_abi_entries_reject_bad_arguments_without_a_gpu():
    lib = _cabi.load()
    assert lib.sage_abi_version() == 22
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    # V pre-pass: head_dim, alignment, sequence count, the slab map all or nothing, its bound
    args = lambda **o: [o.get("v", p), p, p, p, p, p, o.get("sf", None), o.get("ss", None), o.get("hdr", None), o.get("nseq", 2),
                        o.get("total", 100), 64, o.get("bound", 0), 2, o.get("D", 64), o.get("sl", 128), 64, 448.0, 0, None]
    for kw, msg in ((dict(D=96), b"head_dim"), (dict(v=p + 2), b"aligned"), (dict(nseq=0), b"empty"), (dict(sl=130), b"multiples of 8"),
                    (dict(ss=p), b"slab map"), (dict(sf=p, ss=p, hdr=p, bound=0), b"nslab_bound"), (dict(bound=3), b"nslab_bound")):
        rc = lib.sage_prep_v_fp8_varlen(*args(**kw))
        assert rc == -1 and msg in lib.sage_last_error(), (kw, lib.sage_last_error())
    assert lib.sage_prep_v_fp8_varlen_ws_floats(2, 2, 600, 0, 64) == 2 * 2 * 2 * 3 * 64 + 2 * 2 * 3 * 64
    assert lib.sage_prep_v_fp8_varlen_ws_floats(2, 2, 600, 5, 64) == 2 * 5 * 3 * 64 + 2 * 2 * 3 * 64
    assert lib.sage_prep_v_fp8_varlen_ws_floats(0, 2, 600, 5, 64) == 0

    # attention, INT8 q: (q, k, v_image, o, lse, q_scale, k_scale, v_scale, cu_q, cu_k, cu_qs, cu_ks, order, items, hdr, bound,
    #                     nseq, max_seqlen_q, Hq, Hkv, D, q_sl, q_sh, k_sl, k_sh, o_sl, o_sh, lse_sh, causal, sm, accum, out_dtype, stream, attr)
    def int8(**o):
        return lib.sage_attn_qk_int8_pv_f8_varlen(
            o.get("q", p), p, p, p, o.get("lse", None), p, p, o.get("vs", p), p, p, p, p, None, None, None, 0, o.get("nseq", 2), 16, 2, 2,
            o.get("D", 64), 64, 64 * 32, 64, 64 * 32, 64, 64 * 32, o.get("lse_sh", 0), 0, 1.0, o.get("accum", 1), 0, None, o.get("attr", None))
    for kw, msg in ((dict(D=96), b"head_dim"), (dict(q=p + 2), b"aligned"), (dict(nseq=0), b"empty"), (dict(vs=None), b"v_scale"),
                    (dict(accum=2), b"pv_accum"), (dict(lse=p), b"lse_sh")):
        assert int8(**kw) == -1 and msg in lib.sage_last_error(), (kw, lib.sage_last_error())
    folded = _cabi.launch_attr(None, folded_scores=True)
    assert int8(attr=_cabi.attr_arg(folded)) == -1 and b"exact score form" in lib.sage_last_error()

    # attention, fp16 / bf16 q quantised per block in the prologue
    def fused(**o):
        return lib.sage_attn_fused_qblock_pv_f8_varlen(
            o.get("q", p), p, p, p, o.get("lse", None), p, o.get("vs", p), o.get("cu_q", p), p, p, None, None, None, 0, o.get("nseq", 2), 16,
            2, 2, o.get("D", 64), 64, 64 * 32, 64, 64 * 32, 64, 64 * 32, o.get("lse_sh", 0), 0, 1.0, o.get("accum", 1), o.get("qdt", 0), 0,
            None, o.get("attr", None))
    for kw, msg in ((dict(D=96), b"head_dim"), (dict(q=p + 2), b"aligned"), (dict(nseq=0), b"empty"), (dict(vs=None), b"v_scale"),
                    (dict(accum=2), b"pv_accum"), (dict(lse=p), b"lse_sh"), (dict(qdt=5), b"q_dtype"), (dict(cu_q=None), b"cu_seqlens_q")):
        assert fused(**kw) == -1 and msg in lib.sage_last_error(), (kw, lib.sage_last_error())
    assert fused(attr=_cabi.attr_arg(folded)) == -1 and b"exact score form" in lib.sage_last_error()


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_packed_fp8_units_do_not_spill():
    """sage_attn_d{128,64}_f8v.hip: per head size the per-block fused-Q FP8 kernels (fp16 / bf16 q x causal x two-level / single, + the
    four causal ticket-loop instantiations of the work list): no scratch, and the occupancy of the other units (D = 128: 2, D = 64: 3)."""
    import test_build_resources as tbr
    from concurrent.futures import ThreadPoolExecutor
    units = ("sage_attn_d128_f8v.hip", "sage_attn_d64_f8v.hip")
    with ThreadPoolExecutor(max_workers=2) as ex:
        reports = dict(zip(units, ex.map(tbr._resource_report, units)))
    for unit, rep in reports.items():
        mine = {k: v for k, v in rep.items() if "sage_attn_kernel" in k}
        assert len(mine) == 12, (unit, sorted(mine))
        for name, res in mine.items():
            assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0, (unit, name, res)
            assert res["Occupancy"] >= (2 if "128" in unit else 3), (unit, name, res)
