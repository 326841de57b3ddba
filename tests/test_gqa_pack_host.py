"""CPU: the interface of the packed decode launch (``pack_gqa=True``: a GQA group's query heads four to a workgroup) -- the keyword's argument
errors raised before any GPU work, the torch.compile refusal, the flag SAGE_ATTR_GQA_PACK (its value, which entry point takes it and with
which shapes, that the ABI is what it was), the grid arithmetic the launcher and the kernel share, and the build of the kernels behind the
route (units sage_attn_d{128,64}_f8g.hip: instantiation count, zero scratch, the family's occupancy, the MFMA hazard lint)."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

import util  # noqa: F401  (sys.path)
import test_build_resources as tbr
import test_cabi_attn_rejects as rej
from sageattention_amd import _cabi, core as sc
from test_cabi import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("sage_attn_d128_f8g.hip", "sage_attn_d64_f8g.hip")
HONOURED = rej.KVLENS
FLAG = b"SAGE_ATTR_GQA_PACK"


def _cpu_qkv(B=2, Hq=8, Hkv=2, Lq=16, Lk=256, D=64):
    z = lambda h, L: torch.zeros(B, h, L, D, dtype=torch.float16)
    return z(Hq, Lq), z(Hkv, Lk), z(Hkv, Lk)


def _lens(B=2):
    return torch.full((B,), 100, dtype=torch.int32)


ROUTES = [dict(), dict(kv_lens=_lens()), dict(is_causal=True, kv_lens=_lens()), dict(is_causal=True, causal_align="bottom_right", kv_lens=_lens()),
          dict(is_causal=True, q_start=_lens()), dict(is_causal=True, causal_align="bottom_right", window_size=(100, 0))]
ROUTE_IDS = ["plain", "kv_lens", "causal_kv_lens", "bottom_right", "q_start", "window"]


# ---------------------------------------------------------------------------------------------- Python: argument errors
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
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
def test_refused_options_name_themselves_and_the_keyword(route, kw, msg):
    """Everything the kv_lens route refuses is refused with ``pack_gqa`` too, whichever other keywords of the route the call carries, and
    the message names ``pack_gqa`` (its check runs first)."""
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match=msg) as e:
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, pack_gqa=True, **route, **kw)
    assert "pack_gqa" in str(e.value)


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_more_than_32_rows_and_no_group_raise_naming_the_keyword(route):
    for Lq in (33, 64, 129):
        q, k, v = _cpu_qkv(Lq=Lq)
        with pytest.raises(ValueError, match="pack_gqa needs qo_len <= 32"):
            sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, pack_gqa=True, **route)
    for H in (1, 2, 8):
        q, k, v = _cpu_qkv(Hq=H, Hkv=H)
        with pytest.raises(ValueError, match="pack_gqa needs num_qo_heads / num_kv_heads >= 2"):
            sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, pack_gqa=True, **route)
    q, k, v = _cpu_qkv(Lq=16)
    qn, kn, vn = (t.transpose(1, 2).contiguous() for t in (q, k, v))          # NHD: the head and row counts are read per layout
    with pytest.raises(AssertionError, match="cuda"):
        sc.sageattn_qk_int8_pv_fp8_cuda(qn, kn, vn, tensor_layout="NHD", pack_gqa=True, **route)


@pytest.mark.parametrize("bad", [1, 0, "yes", "True", 1.0, [True]])
def test_the_keyword_is_a_bool_or_none(bad):
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match="pack_gqa must be None, False or True"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, pack_gqa=bad)


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("Lq", [1, 5, 32])
@pytest.mark.parametrize("heads", [(8, 2), (6, 2), (10, 2), (2, 1)])
def test_supported_calls_pass_the_argument_check(route, Lq, heads):
    q, k, v = _cpu_qkv(Hq=heads[0], Hkv=heads[1], Lq=Lq)
    for kw in (dict(), dict(pv_accum_dtype="fp32+fp32", smooth_k=False, split_kv=0)):
        with pytest.raises(AssertionError, match="cuda"):        # (accepted; then the ordinary input check of a CPU tensor)
            sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, pack_gqa=True, **route, **kw)


@pytest.mark.parametrize("off", [None, False])
def test_off_is_the_call_without_the_keyword(off):
    """None / False ask for nothing: no restriction of the route applies (more than 32 rows, no group, the folded score form ...)."""
    q, k, v = _cpu_qkv(Hq=2, Hkv=2, Lq=64)
    with pytest.raises(AssertionError, match="cuda"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, pack_gqa=off, fp8_scores="folded", pv_accum_dtype="fp32")


def test_torch_compile_refuses_the_keyword(monkeypatch):
    q, k, v = _cpu_qkv()
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    for fn in (sc.sageattn_qk_int8_pv_fp8_cuda, sc.sageattn):
        with pytest.raises(ValueError, match="pack_gqa is not supported under torch.compile"):
            fn(q, k, v, pack_gqa=True)


def test_the_keyword_is_a_named_parameter_and_sageattn_forwards_it():
    import sageattention
    assert sageattention.sageattn_qk_int8_pv_fp8_cuda is sc.sageattn_qk_int8_pv_fp8_cuda
    for fn in (sc.sageattn_qk_int8_pv_fp8_cuda, sc.sageattn):
        par = inspect.signature(fn).parameters
        assert par["pack_gqa"].default is None and list(par)[-1] == "kwargs"
        assert "pack_gqa" in fn.__doc__
    assert "pack_gqa=pack_gqa" in inspect.getsource(sc.sageattn)
    q, k, v = _cpu_qkv(Lq=33)
    with pytest.raises(ValueError, match="pack_gqa needs qo_len <= 32"):          # (checked before any work: not the input check's "cuda")
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, pack_gqa=True)
    q, k, v = _cpu_qkv()
    for route in ROUTES:                                                          # with lengths, with offsets, alone: every route is told to pack
        kw = dict(dict(is_causal=False, kv_lens=None, q_start=None, causal_align="top_left", window_size=None), **route)
        call = sc._kv_family_args(q, k, "HND", kw["is_causal"], kw["kv_lens"], kw["q_start"], kw["causal_align"], kw["window_size"], True, None,
                                  "per_thread", "fp32+fp16", False, {})
        assert call.gqa_pack is True


# ---------------------------------------------------------------------------------------------- C ABI: the flag
def test_the_define_equals_the_mirror_and_the_abi_is_unchanged():
    lib = _cabi.load()
    header = open(os.path.join(ROOT, "include", "sage_gfx950.h")).read()
    m = re.search(r"^#define\s+SAGE_ATTR_GQA_PACK\s+0x([0-9a-fA-F]+)u\s*$", header, re.M)
    assert m and int(m.group(1), 16) == _cabi.ATTR_GQA_PACK == 0x100
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22 and len(prototypes()) == 56 and len(_cabi.SYMBOLS) == 56
    assert ctypes.sizeof(_cabi.SageLaunchAttr) == 56 and [f[0] for f in _cabi.SageLaunchAttr._fields_][-2:] == ["window", "q_start"]
    assert len(rej.ATTN) == 17
    assert re.search(r"^ \*  flags bit 0x100\s+SAGE_ATTR_GQA_PACK", header, re.M), "the header's attribute block documents the flag"


def test_launch_attr_carries_the_flag():
    assert _cabi.launch_attr() is None and _cabi.launch_attr(gqa_pack=False) is None
    a = _cabi.launch_attr(gqa_pack=True)
    assert a is not None and a.flags == 0x100 and a.struct_bytes == 56 and a.window == 0 and not a.q_start and not a.launch_ws
    assert _cabi.launch_attr(gqa_pack=True, causal_bottom_right=True).flags == 0x108
    assert _cabi.launch_attr(window=5).flags == 0
    from sageattention_amd import ops
    assert "gqa_pack" in inspect.signature(ops.attn_attr).parameters
    src = inspect.getsource(sc._attn_fused_q)
    assert "gqa_pack=gqa_pack" in src and inspect.signature(sc._attn_fused_q).parameters["gqa_pack"].default is False


def _call(name, flags, **wrong):
    """``name`` with the refusal table's valid arguments (host memory: the library must refuse before its first HIP call) but for ``wrong``."""
    attr = _cabi.SageLaunchAttr(struct_bytes=ctypes.sizeof(_cabi.SageLaunchAttr), flags=flags)
    args = []
    for ctype, pname in prototypes()[name][1]:
        args.append(wrong[pname] if pname in wrong else rej.VALID[pname] if pname in rej.VALID else rej.P)
    args[-1] = ctypes.byref(attr)
    lib = _cabi.load()
    return getattr(lib, name)(*args), lib.sage_last_error()


@pytest.mark.parametrize("name", [n for n in rej.ATTN if n != HONOURED])
@pytest.mark.parametrize("causal", [0, 1])
def test_every_other_entry_point_refuses_the_flag(name, causal):
    """Sixteen entries, the exact split's own attribute path included -- also with decode shapes, which are not what they refuse."""
    for shape in (dict(), dict(Lq=16, max_seqlen_q=16)):
        rc, err = _call(name, _cabi.ATTR_GQA_PACK, **shape, **({} if name.endswith("_masked") else dict(is_causal=causal)))
        assert rc == -1 and FLAG in err, (rc, err)


def test_sixteen_entries_refuse_and_one_honours():
    assert HONOURED in rej.ATTN and len([n for n in rej.ATTN if n != HONOURED]) == 16 and rej.EXACT in rej.ATTN


@pytest.mark.parametrize("causal", [0, 1])
def test_the_honoured_entry_refuses_the_flag_where_the_route_does_not_exist(causal):
    for wrong, piece in ((dict(Lq=33), b"Lq <= 32"), (dict(Lq=128), b"Lq <= 32"), (dict(Lq=16, Hq=2, Hkv=2), b"Hq / Hkv >= 2"),
                         (dict(Lq=16, Hq=1, Hkv=1), b"Hq / Hkv >= 2")):
        rc, err = _call(HONOURED, _cabi.ATTR_GQA_PACK, is_causal=causal, **wrong)
        assert rc == -1 and FLAG in err and piece in err, (wrong, rc, err)
    rc, err = _call(HONOURED, _cabi.ATTR_GQA_PACK | _cabi.ATTR_FP8_FOLDED_SCORES, is_causal=causal, Lq=16)
    assert rc == -1 and FLAG in err and b"exact score form" in err, (rc, err)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("Lq", [1, 16, 32])
def test_the_honoured_entry_takes_the_flag_as_far_as_the_checks_go(causal, Lq):
    """Decode-shaped, a group of two, the exact form: the next refusal is the one asked for (head_dim 96), not the flag's -- the tensors are
    host memory."""
    for flags in (_cabi.ATTR_GQA_PACK, _cabi.ATTR_GQA_PACK | _cabi.ATTR_FP8_EXACT_SCORES):
        rc, err = _call(HONOURED, flags, is_causal=causal, Lq=Lq, D=96)
        assert rc == -1 and b"head_dim must be 64 or 128 (got 96)" in err and FLAG not in err, (rc, err)
    if causal:                                                  # ... with a window (and offsets left null) as well
        attr = _cabi.SageLaunchAttr(struct_bytes=ctypes.sizeof(_cabi.SageLaunchAttr), flags=_cabi.ATTR_GQA_PACK, window=100)
        args = [dict(is_causal=1, Lq=Lq, D=96).get(p, rej.VALID[p] if p in rej.VALID else rej.P) for _, p in prototypes()[HONOURED][1]]
        args[-1] = ctypes.byref(attr)
        lib = _cabi.load()
        assert getattr(lib, HONOURED)(*args) == -1 and b"head_dim must be 64 or 128 (got 96)" in lib.sage_last_error()


@pytest.mark.parametrize("name", rej.ATTN)
def test_the_bits_around_it_stay_unknown(name):
    for bit in (0x10, 0x20, 0x40, 0x80, 0x200, 0x400):
        for flags in (bit, bit | _cabi.ATTR_GQA_PACK):
            rc, err = _call(name, flags, Lq=16, max_seqlen_q=16, **({} if name.endswith("_masked") else dict(is_causal=1)))
            assert rc == -1 and b"unknown SageLaunchAttr.flags" in err, (name, hex(flags), rc, err)


# ---------------------------------------------------------------------------------------------- the grid
def test_the_packed_grid_covers_every_head_once():
    """The kernel's decode of a workgroup index, restated: index u of B * Hkv * ceil(group / 4) -> (b, hk, block); wave w serves head
    hk * group + 4 * block + w when 4 * block + w < group.  Every (b, query head) is served by exactly one wave, and no head index reaches Hq."""
    for B, Hq, Hkv in ((3, 8, 2), (3, 6, 2), (1, 16, 2), (2, 10, 2), (1, 2, 1), (2, 7, 1), (1, 64, 8)):
        group = Hq // Hkv
        ngb = (group + 3) // 4
        seen = {}
        for u in range(B * Hkv * ngb):
            bk, gb = divmod(u, ngb)
            b, hk = divmod(bk, Hkv)
            for w in range(4):
                hw = 4 * gb + w
                if hw < group:
                    h = hk * group + hw
                    assert 0 <= h < Hq and (b, h) not in seen
                    seen[(b, h)] = (u, w)
        assert len(seen) == B * Hq


# ---------------------------------------------------------------------------------------------- the build
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_gpack_units_build_within_the_family_targets():
    """The units are in the Makefile's SRCS; each holds eight kernels -- fp16 / bf16 q x {non-causal lengths, causal lengths, offsets, offsets
    with a window} -- with the GPACK flag on top of the family's form: zero scratch, no spilled VGPR, D = 128 at two waves per
    SIMD, D = 64 at three."""
    mk = open(os.path.join(ROOT, "sageattention_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert all(u in srcs for u in UNITS), srcs
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as ex:
        reports = dict(zip(UNITS, ex.map(tbr._resource_report, UNITS)))
    for unit, rep in reports.items():
        mine = {k: v for k, v in rep.items() if "sage_attn_kernel" in k}
        assert len(mine) == 8, (unit, sorted(mine))
        d128 = "d128" in unit
        forms = set()
        for name, res in mine.items():
            # D, FP8 PV, causal or not, per-thread k scales, two-level, no mask, QF 1 / 2, GPACK, the exact form, no CPERS / VROWS / SEED ... KVLEN
            f = tbr.kf.decode(name)
            assert f["qf"] in (1, 2) and f == tbr.kf.form(128 if d128 else 64, pv_fp8=True, kthread=True, two_level=True, gpack=True, kvlen=True,
                                                          causal=f["causal"], qf=f["qf"], window=f["window"], qstart=f["qstart"]), name
            forms.add((f["causal"], f["qf"], f["window"], f["qstart"]))
            assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0, (name, res)
            assert res["Occupancy"] >= (2 if d128 else 3) and res["VGPRs"] <= (256 if d128 else 168), (name, res)
        # (causal, QF, WINDOW, QSTART)
        assert forms == {(c, f, w, s) for f in (1, 2) for c, w, s in ((False, False, False), (True, False, False), (True, False, True), (True, True, True))}, sorted(forms)


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_gpack_units_pass_the_mfma_hazard_lint():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_hazard_lint as lint
    assert lint.UNITS_GQA_PACK == UNITS
    assert not set(UNITS) & set(lint.UNITS + lint.UNITS_PAIR + lint.UNITS_WINDOW + lint.UNITS_PACKED_BR + lint.UNITS_PACKED_WINDOW)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as ex:
        results = dict(zip(UNITS, ex.map(lambda u: lint.lint(lint.listing(u)), UNITS)))
    for unit, (findings, n_mfma) in results.items():
        assert n_mfma >= 400, (unit, n_mfma)                   # (eight kernels: the walk did see the pipelined loops)
        assert not findings, (unit, findings[:5])
