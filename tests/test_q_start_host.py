"""CPU: the interface of per-sample query offsets (``q_start`` / ``causal_align``) -- the keyword and tensor errors raised before any GPU
work, the torch.compile refusal, the field appended to ``SageLaunchAttr`` under the unchanged ABI version (which entry point takes it, that an
older caller's shorter struct still passes), and the build of the kernels behind the route (units sage_attn_d{128,64}_f8q.hip: instantiation
count, zero scratch, the family's occupancy, the MFMA hazard lint)."""
import ctypes
import os
import re
import sys

import pytest
import torch

import util  # noqa: F401  (sys.path)
import test_build_resources as tbr
import test_cabi_attn_rejects as rej
from sageattention_amd import _cabi, core as sc, processors
from test_cabi import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("sage_attn_d128_f8q.hip", "sage_attn_d64_f8q.hip")


def _cpu_qkv(B=2, Lk=256, D=64):
    z = lambda L: torch.zeros(B, 2, L, D, dtype=torch.float16)
    return z(16), z(Lk), z(Lk)


def _starts(B=2, dtype=torch.int32):
    return torch.full((B,), 100, dtype=dtype)


KEYWORDS = [dict(q_start=_starts()), dict(q_start=7), dict(causal_align="bottom_right")]
KW_IDS = ["tensor", "int", "bottom_right"]


# ---------------------------------------------------------------------------------------------- Python: argument errors
@pytest.mark.parametrize("given", KEYWORDS, ids=KW_IDS)
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
def test_refused_options_name_themselves_and_the_keyword(given, kw, msg):
    q, k, v = _cpu_qkv()
    name = "q_start" if "q_start" in given else "causal_align"
    with pytest.raises(ValueError, match=msg) as e:
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=True, **given, **kw)
    assert name in str(e.value)


@pytest.mark.parametrize("given", KEYWORDS, ids=KW_IDS)
def test_not_causal_raises(given):
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match="is_causal=True"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, **given)
    with pytest.raises(ValueError, match="is_causal=True"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, kv_lens=_starts(), **given)


def test_both_keywords_raise_and_the_alignment_is_one_of_two():
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match="either q_start or causal_align"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=True, q_start=_starts(), causal_align="bottom_right")
    with pytest.raises(ValueError, match="either q_start or causal_align"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=True, q_start=0, causal_align="bottom_right")
    for bad in ("bottom_left", "", None, True):
        with pytest.raises(ValueError, match="causal_align must be"):
            sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=True, causal_align=bad)


@pytest.mark.parametrize("bad,msg", [
    (lambda: torch.full((2,), 100, dtype=torch.int16), "int32 / int64"),
    (lambda: torch.full((2,), 100.0), "int32 / int64"),
    (lambda: torch.full((2,), True), "int32 / int64"),
    (lambda: [100, 100], "int32 / int64"),
    (lambda: 100.0, "int32 / int64"),
    (lambda: True, "int32 / int64"),
    (lambda: torch.full((2, 1), 100, dtype=torch.int32), "shape"),
    (lambda: torch.tensor(100, dtype=torch.int32), "shape"),
    (lambda: torch.full((3,), 100, dtype=torch.int32), "shape"),
    (lambda: torch.full((2,), 100, dtype=torch.int32, device="meta"), "device"),
])
def test_a_bad_q_start_raises(bad, msg):
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match=msg):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=True, q_start=bad())


@pytest.mark.parametrize("given", KEYWORDS + [dict(q_start=_starts(dtype=torch.int64)), dict(q_start=-5), dict(causal_align="top_left")],
                         ids=KW_IDS + ["int64", "negative_int", "top_left"])
@pytest.mark.parametrize("kw", [dict(), dict(split_kv=None), dict(split_kv=0), dict(pv_accum_dtype="fp32+fp32"), dict(smooth_k=False),
                                dict(kv_lens=_starts())], ids=["default", "split_none", "split_0", "fp32+fp32", "nosk", "kv_lens"])
def test_supported_options_pass_the_argument_check(given, kw):
    q, k, v = _cpu_qkv()
    with pytest.raises(AssertionError, match="cuda"):        # (accepted; then the ordinary input check of a CPU tensor)
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=True, **given, **kw)


@pytest.mark.parametrize("given", KEYWORDS, ids=KW_IDS)
def test_torch_compile_refuses_the_keywords(monkeypatch, given):
    """The compiled op takes the default routes and sageattn's compiling branch forwards no keyword: a given offset is an error in both."""
    q, k, v = _cpu_qkv()
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    for fn in (sc.sageattn_qk_int8_pv_fp8_cuda, sc.sageattn, processors.sdpa):
        with pytest.raises(ValueError, match="q_start / causal_align are not supported under torch.compile"):
            fn(q, k, v, is_causal=True, **given)


def test_sdpa_takes_a_mask_or_offsets_and_the_mirror_package_has_the_keywords():
    import inspect
    import sageattention
    q, k, v = _cpu_qkv()
    for given in KEYWORDS:
        with pytest.raises(ValueError, match="attn_mask or q_start / causal_align"):
            processors.sdpa(q, k, v, attn_mask=torch.ones(16, 256, dtype=torch.bool), is_causal=True, **given)
    for fn in (sageattention.sageattn, sageattention.sageattn_qk_int8_pv_fp8_cuda, sc.sageattn, processors.sdpa):
        assert {"q_start", "causal_align"} <= set(inspect.signature(fn).parameters), fn
    assert sageattention.sageattn is sc.sageattn


def test_bottom_right_offsets_are_formed_without_a_host_read():
    """clamp(kv_lens, 0, Lk) - Lq by tensor ops on the lengths' device (a meta tensor has no data to read); constants otherwise."""
    lens = torch.empty(3, dtype=torch.int64, device="meta")
    s = sc._q_start_tensor(None, lens, 3, 200, 640, lens.device)
    assert s.device.type == "meta" and s.dtype == torch.int32 and s.shape == (3,)
    s = sc._q_start_tensor(torch.empty(3, dtype=torch.int64, device="meta"), None, 3, 200, 640, lens.device)
    assert s.device.type == "meta" and s.dtype == torch.int32
    assert sc._q_start_tensor(None, torch.tensor([700, 640, 100, 0, -4]), 5, 200, 640, "cpu").tolist() == [440, 440, -100, -200, -200]
    assert sc._q_start_tensor(None, None, 2, 200, 640, "cpu").tolist() == [440, 440]
    assert sc._q_start_tensor(-3, None, 2, 200, 640, "cpu").tolist() == [-3, -3]
    assert sc._q_start_tensor(torch.tensor([2 ** 40, -2 ** 40, 5]), None, 3, 200, 640, "cpu").tolist() == [2 ** 31 - 1, -2 ** 31, 5]


# ---------------------------------------------------------------------------------------------- C ABI
def test_abi_version_and_prototype_count_are_unchanged():
    lib = _cabi.load()
    header = open(os.path.join(ROOT, "include", "sage_gfx950.h")).read()
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22 and "#define SAGE_ABI_VERSION 22" in header
    assert len(prototypes()) == 56 and len(_cabi.SYMBOLS) == 56
    assert len(rej.ATTN) == 17
    # the field is the struct's last, in the header and in its mirror
    body = re.search(r"typedef struct SageLaunchAttr \{(.*?)\} SageLaunchAttr;", header, re.S).group(1)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert fields[-1] == "const int32_t *q_start" and len(fields) == len(_cabi.SageLaunchAttr._fields_)
    assert _cabi.SageLaunchAttr._fields_[-1][0] == "q_start" and _cabi.SageLaunchAttr.q_start.offset == 48
    assert ctypes.sizeof(_cabi.SageLaunchAttr) == 56


def _call(name, attr, **wrong):
    """``name`` with the refusal table's valid arguments (host memory: the library must refuse before its first HIP call) but for ``wrong``."""
    args = []
    for ctype, pname in prototypes()[name][1]:
        v = wrong[pname] if pname in wrong else rej.VALID[pname] if pname in rej.VALID else rej.P
        args.append(v)
    args[-1] = ctypes.byref(attr) if attr is not None else None
    lib = _cabi.load()
    return getattr(lib, name)(*args), lib.sage_last_error()


def _attr(q_start=rej.P, flags=0, struct_bytes=None):
    a = _cabi.SageLaunchAttr()
    a.struct_bytes = ctypes.sizeof(a) if struct_bytes is None else struct_bytes
    a.flags = flags
    a.q_start = q_start
    return a


@pytest.mark.parametrize("name", [n for n in rej.ATTN if n != rej.KVLENS])
@pytest.mark.parametrize("causal", [0, 1])
def test_every_other_entry_point_refuses_q_start(name, causal):
    rc, err = _call(name, _attr(), **({} if name.endswith("_masked") else dict(is_causal=causal)))
    assert rc == -1 and b"q_start" in err, (rc, err)


def test_the_kvlens_entry_refuses_q_start_without_causal_and_with_folded_scores():
    rc, err = _call(rej.KVLENS, _attr(), is_causal=0)
    assert rc == -1 and b"q_start" in err and b"is_causal = 1" in err, (rc, err)
    rc, err = _call(rej.KVLENS, _attr(flags=_cabi.ATTR_FP8_FOLDED_SCORES), is_causal=1)
    assert rc == -1 and b"q_start" in err, (rc, err)
    # causal and exact: accepted as far as the checks go (the next refusal is the one asked for, not q_start's)
    rc, err = _call(rej.KVLENS, _attr(), is_causal=1, D=96)
    assert rc == -1 and b"head_dim" in err and b"q_start" not in err, (rc, err)


@pytest.mark.parametrize("name", rej.ATTN)
def test_a_null_q_start_and_an_older_struct_change_nothing(name):
    """A struct of the size before the field (48 bytes) is read as far as it goes: what lies behind it -- here a non-null pointer -- is not
    seen.  The call goes on to the refusal asked for (head_dim 96): the tensors are host memory, so no call here may be accepted."""
    for attr in (_attr(q_start=None), _attr(struct_bytes=48), _attr(struct_bytes=52), _attr(struct_bytes=8)):      # (52: ends inside the field)
        rc, err = _call(name, attr, D=96)
        assert rc == -1 and b"head_dim must be 64 or 128 (got 96)" in err, (rc, err)


def test_launch_attr_carries_the_offsets():
    assert _cabi.launch_attr() is None
    t = torch.zeros(4, dtype=torch.int32)
    a = _cabi.launch_attr(q_start=t)
    assert a is not None and a.q_start == t.data_ptr() and a.struct_bytes == 56 and a.flags == 0 and not a.launch_ws


# ---------------------------------------------------------------------------------------------- the build
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_qstart_units_build_within_the_family_targets():
    """The units are in the Makefile's SRCS (so the whole-library scratch check sees them); each holds the causal kernel for fp16 and for
    bf16 q -- the offset places a causal diagonal, there is no non-causal member: four kernels over the two units -- with zero scratch,
    D = 128 at two waves per SIMD, D = 64 at three."""
    mk = open(os.path.join(ROOT, "sageattention_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert all(u in srcs for u in UNITS), srcs
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as ex:
        reports = dict(zip(UNITS, ex.map(tbr._resource_report, UNITS)))
    for unit, rep in reports.items():
        mine = {k: v for k, v in rep.items() if "sage_attn_kernel" in k}
        assert len(mine) == 2, (unit, sorted(mine))
        d128 = "d128" in unit
        forms = {name: tbr.kf.decode(name) for name in mine}
        for name, res in mine.items():
            # D, FP8 PV, causal, per-thread, two-level, the exact form ... QSTART, KVLEN and nothing else
            assert forms[name] == tbr.kf.form(128 if d128 else 64, pv_fp8=True, causal=True, kthread=True, two_level=True, qstart=True, kvlen=True,
                                              qf=forms[name]["qf"]), name
            assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0, (name, res)
            assert res["Occupancy"] >= (2 if d128 else 3) and res["VGPRs"] <= (256 if d128 else 168), (name, res)
        assert {f["qf"] for f in forms.values()} == {1, 2}, sorted(mine)      # (QF 1 and 2: fp16, bf16)


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_qstart_units_pass_the_mfma_hazard_lint():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_hazard_lint as lint
    assert lint.UNITS_PAIR == UNITS
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as ex:
        results = dict(zip(UNITS, ex.map(lambda u: lint.lint(lint.listing(u)), UNITS)))
    for unit, (findings, n_mfma) in results.items():
        assert n_mfma >= 100, (unit, n_mfma)                   # (two kernels: the walk did see the pipelined loops)
        assert not findings, (unit, findings[:5])
