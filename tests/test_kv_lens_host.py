"""CPU: the interface of per-sample key lengths (``kv_lens``) -- the new C-ABI symbols under the unchanged ABI version, the keyword and tensor
errors raised before any GPU work, the torch.compile refusal, the C ABI's own argument checks, and the build of the kernels behind the route
(units sage_attn_d{128,64}_f8k.hip: instantiation count, zero scratch, the family's occupancy, the MFMA hazard lint)."""
import ctypes
import os
import re
import sys

import pytest
import torch

import util  # noqa: F401  (sys.path)
import test_build_resources as tbr
from sageattention_amd import _cabi, core as sc, processors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("sage_attn_d128_f8k.hip", "sage_attn_d64_f8k.hip")
NEW_SYMBOLS = ("sage_channel_mean_kvlens", "sage_quant_qk_int8_kvlens", "sage_prep_v_fp8_kvlens", "sage_attn_fused_q_pv_f8_kvlens")


def _cpu_qkv(B=2, Lk=256, D=64):
    z = lambda L: torch.zeros(B, 2, L, D, dtype=torch.float16)
    return z(16), z(Lk), z(Lk)


def _lens(B=2, dtype=torch.int32):
    return torch.full((B,), 100, dtype=dtype)


def test_symbols_and_abi_version():
    lib = _cabi.load()
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22
    header = open(os.path.join(ROOT, "include", "sage_gfx950.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _cabi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"SAGE_API int %s\(" % name, header), name
    assert "#define SAGE_ABI_VERSION 22" in header


@pytest.mark.parametrize("kw,msg", [
    (dict(qk_quant_gran="per_warp"), "qk_quant_gran"),
    (dict(qk_quant_gran="per_block"), "qk_quant_gran"),
    (dict(pv_accum_dtype="fp32"), "pv_accum_dtype"),
    (dict(fuse_q_quant=False), "fuse_q_quant"),
    (dict(fp8_scores="folded"), "fp8_scores"),
    (dict(smooth_v=True), "smooth_v"),
    (dict(split_kv=2), "split_kv"),
    (dict(split_kv="auto"), "split_kv"),
    (dict(split_kv_exact=True), "split_kv_exact"),
])
def test_refused_options_name_themselves(kw, msg):
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match=msg):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, kv_lens=_lens(), **kw)


@pytest.mark.parametrize("kw", [dict(), dict(split_kv=None), dict(split_kv=0), dict(pv_accum_dtype="fp32+fp32"), dict(smooth_k=False)])
def test_supported_options_pass_the_argument_check(kw):
    q, k, v = _cpu_qkv()
    for dtype in (torch.int32, torch.int64):
        with pytest.raises(AssertionError, match="cuda"):        # (accepted; then the ordinary input check of a CPU tensor)
            sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, kv_lens=_lens(dtype=dtype), **kw)


@pytest.mark.parametrize("bad,msg", [
    (lambda: torch.full((2,), 100, dtype=torch.int16), "int32 or int64"),
    (lambda: torch.full((2,), 100.0), "int32 or int64"),
    (lambda: torch.full((2,), True), "int32 or int64"),
    (lambda: [100, 100], "int32 or int64"),
    (lambda: torch.full((2, 1), 100, dtype=torch.int32), "shape"),
    (lambda: torch.tensor(100, dtype=torch.int32), "shape"),
    (lambda: torch.full((3,), 100, dtype=torch.int32), "shape"),
    (lambda: torch.full((2,), 100, dtype=torch.int32, device="meta"), "device"),
])
def test_a_bad_kv_lens_tensor_raises(bad, msg):
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match=msg):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, kv_lens=bad())


def test_torch_compile_refuses_kv_lens(monkeypatch):
    """The compiled op takes the default routes and sageattn's compiling branch forwards no keyword: a given kv_lens is an error in both."""
    q, k, v = _cpu_qkv()
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    with pytest.raises(ValueError, match="kv_lens"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, kv_lens=_lens())
    with pytest.raises(ValueError, match="kv_lens"):
        sc.sageattn(q, k, v, kv_lens=_lens())
    with pytest.raises(ValueError, match="kv_lens"):
        processors.sdpa(q, k, v, kv_lens=_lens())


def test_sdpa_takes_a_mask_or_lengths():
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match="attn_mask or kv_lens"):
        processors.sdpa(q, k, v, attn_mask=torch.ones(16, 256, dtype=torch.bool), kv_lens=_lens())


def test_cabi_refuses_null_lengths_and_what_the_plain_entries_refuse():
    lib = _cabi.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    B, H, L, D = 1, 1, 64, 64
    st = (H * L * D, L * D, D)
    attn = lambda lens, D_=D, attr=None: lib.sage_attn_fused_q_pv_f8_kvlens(p, p, p, p, None, p, p, None, lens, B, H, H, 16, L, D_, *st, *st, *st,
                                                                            0, 1.0, 0, 0, None, attr)
    assert attn(None) == -1 and b"kv_lens" in lib.sage_last_error()
    assert attn(p, D_=96) == -1 and b"head_dim" in lib.sage_last_error()
    folded = _cabi.launch_attr(folded_scores=True)
    assert attn(p, attr=_cabi.attr_arg(folded)) == -1 and b"kv_lens" in lib.sage_last_error()
    assert lib.sage_channel_mean_kvlens(p, p, p, None, B, H, L, D, *st, 0, None) == -1 and b"kv_lens" in lib.sage_last_error()
    assert lib.sage_channel_mean_kvlens(p, p, p, p, B, H, L, 96, *st, 0, None) == -1
    assert lib.sage_quant_qk_int8_kvlens(p, None, p, p, None, B, H, L, D, *st, *st, 0, 0, 0, None) == -1 and b"kv_lens" in lib.sage_last_error()
    assert lib.sage_quant_qk_int8_kvlens(p, None, p, p, p, B, H, L, D, *st, *st, 0, 0, 7, None) == -1 and b"dtype" in lib.sage_last_error()
    assert lib.sage_prep_v_fp8_kvlens(p, p, p, p, None, B, H, L, D, *st, 448.0, 0, None) == -1 and b"kv_lens" in lib.sage_last_error()
    assert lib.sage_prep_v_fp8_kvlens(p, p, p, p, p, B, H, L, D, *st, 0.0, 0, None) == -1 and b"scale_max" in lib.sage_last_error()


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_kvlens_units_build_within_the_family_targets():
    """The units are in the Makefile's SRCS (so the whole-library scratch check sees them); each holds four instantiations of the attention
    kernel -- causal / non-causal x fp16 / bf16 q -- with zero scratch, D = 128 at two waves per SIMD, D = 64 at three."""
    mk = open(os.path.join(ROOT, "sageattention_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert all(u in srcs for u in UNITS), srcs
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as ex:
        reports = dict(zip(UNITS, ex.map(tbr._resource_report, UNITS)))
    for unit, rep in reports.items():
        mine = {k: v for k, v in rep.items() if "sage_attn_kernel" in k}
        assert len(mine) == 4, (unit, sorted(mine))
        d128 = "d128" in unit
        for name, res in mine.items():
            f = tbr.kf.decode(name)      # (the fused per-thread Q FP8 kernels with KVLEN and nothing else; causal or not, fp16 / bf16 q)
            assert f["qf"] in (1, 2) and f == tbr.kf.form(128 if d128 else 64, pv_fp8=True, kthread=True, two_level=True, kvlen=True, causal=f["causal"], qf=f["qf"]), name
            assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0, (name, res)
            assert res["Occupancy"] >= (2 if d128 else 3) and res["VGPRs"] <= (256 if d128 else 168), (name, res)


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_kvlens_units_pass_the_mfma_hazard_lint():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_hazard_lint as lint
    assert all(u in lint.UNITS for u in UNITS)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as ex:
        results = dict(zip(UNITS, ex.map(lambda u: lint.lint(lint.listing(u)), UNITS)))
    for unit, (findings, n_mfma) in results.items():
        assert n_mfma >= 200, (unit, n_mfma)
        assert not findings, (unit, findings[:5])
