"""CPU: bottom-right causal alignment of the packed FP8-PV route (``sageattn_qk_int8_pv_fp8_varlen(causal_align="bottom_right")``) -- the
keyword's argument errors, the flag SAGE_ATTR_CAUSAL_BOTTOM_RIGHT (which entry point takes it, with which arguments, and that the bits above
it stay unknown), the work list under the bottom-right weights (``sage_debug_varlen_items(is_causal=2)`` against a brute-force sort), the
kernel's loop bounds restated in Python against the predicate, and the build of the kernels behind the route (units
sage_attn_d{128,64}_f8vb.hip: instantiation count, zero scratch, the family's occupancy, the MFMA hazard lint)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import util  # noqa: F401  (sys.path)
import ref_varlen_br as rb
import test_build_resources as tbr
import test_cabi_attn_rejects as rej
from sageattention_amd import _cabi, core as sc
from test_cabi import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("sage_attn_d128_f8vb.hip", "sage_attn_d64_f8vb.hip")
HONOURED = "sage_attn_fused_qblock_pv_f8_varlen"
FLAG = b"SAGE_ATTR_CAUSAL_BOTTOM_RIGHT"


# ---------------------------------------------------------------------------------------------- Python: argument errors
def _cpu_packed():
    z = lambda n, h: torch.zeros(n, h, 64, dtype=torch.float16)
    cu_q, cu_k = torch.tensor([0, 16, 48], dtype=torch.int32), torch.tensor([0, 100, 256], dtype=torch.int32)
    return (z(48, 4), z(256, 2), z(256, 2), cu_q, cu_k, 32, 156)


@pytest.mark.parametrize("kw,msg", [
    (dict(is_causal=False), "is_causal"),
    (dict(is_causal=True, pv_accum_dtype="fp32"), "pv_accum_dtype"),
    (dict(is_causal=True, fuse_q_quant=False), "fuse_q_quant"),
])
def test_refused_options_name_themselves_and_the_keyword(kw, msg):
    with pytest.raises(ValueError, match=msg) as e:
        sc.sageattn_qk_int8_pv_fp8_varlen(*_cpu_packed(), causal_align="bottom_right", **kw)
    assert "causal_align" in str(e.value)


@pytest.mark.parametrize("value", ["bottom-right", "BOTTOM_RIGHT", "top_right", "", None, 1, True])
@pytest.mark.parametrize("causal", [False, True])
def test_an_unknown_alignment_raises(value, causal):
    with pytest.raises(ValueError, match="causal_align"):
        sc.sageattn_qk_int8_pv_fp8_varlen(*_cpu_packed(), is_causal=causal, causal_align=value)


@pytest.mark.parametrize("kw", [dict(causal_align="bottom_right", is_causal=True), dict(causal_align="bottom_right", is_causal=True, smooth_k=False),
                                dict(causal_align="bottom_right", is_causal=True, return_lse=True, work_list=False, varlen_plan=False, fused_prepass=False),
                                dict(causal_align="top_left", is_causal=False), dict(causal_align="top_left", is_causal=True, pv_accum_dtype="fp32"),
                                dict(causal_align="top_left", is_causal=True, fuse_q_quant=False), dict()])
def test_supported_options_pass_the_argument_check(kw):
    with pytest.raises(AssertionError, match="cuda"):        # (accepted; then the ordinary input check of a CPU tensor)
        sc.sageattn_qk_int8_pv_fp8_varlen(*_cpu_packed(), **kw)


def test_the_keyword_is_read_by_name_and_the_mirror_package_has_the_function():
    """The parameter list of the function is pinned (tests/test_varlen_fp8_host.py::test_signature_and_defaults ends it with ``**kwargs``), so
    the keyword arrives there: it is taken out by name, validated before anything else looks at ``kwargs``, and documented."""
    import sageattention
    assert sageattention.sageattn_qk_int8_pv_fp8_varlen is sc.sageattn_qk_int8_pv_fp8_varlen
    sig = inspect.signature(sc.sageattn_qk_int8_pv_fp8_varlen)
    assert list(sig.parameters)[-1] == "kwargs" and sig.parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    doc = sc.sageattn_qk_int8_pv_fp8_varlen.__doc__
    assert "causal_align" in doc and "bottom_right" in doc and "top_left" in doc
    src = inspect.getsource(sc.sageattn_qk_int8_pv_fp8_varlen)
    assert src.index('kwargs.pop("causal_align"') < src.index("_varlen_prepare(")
    assert "causal_align" not in (sc.sageattn_varlen.__doc__ or "")                          # (FP16 PV, the reference's name: unchanged)


# ---------------------------------------------------------------------------------------------- C ABI: the flag
def test_the_define_equals_the_mirror_and_the_abi_is_unchanged():
    lib = _cabi.load()
    header = open(os.path.join(ROOT, "include", "sage_gfx950.h")).read()
    m = re.search(r"^#define\s+SAGE_ATTR_CAUSAL_BOTTOM_RIGHT\s+(\d+)u\s*$", header, re.M)
    assert m and int(m.group(1)) == _cabi.ATTR_CAUSAL_BOTTOM_RIGHT == 8
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22 and len(prototypes()) == 56 and len(_cabi.SYMBOLS) == 56
    assert ctypes.sizeof(_cabi.SageLaunchAttr) == 56 and [f[0] for f in _cabi.SageLaunchAttr._fields_][-2:] == ["window", "q_start"]
    assert re.search(r"^ \*  flags bit 8\s+SAGE_ATTR_CAUSAL_BOTTOM_RIGHT", header, re.M), "the header's attribute block documents the flag"


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
    """(The exact split has an attribute path of its own; it is one of the sixteen.)"""
    rc, err = _call(name, _cabi.ATTR_CAUSAL_BOTTOM_RIGHT, **({} if name.endswith("_masked") else dict(is_causal=causal)))
    assert rc == -1 and FLAG in err, (rc, err)


def test_sixteen_entries_refuse_and_one_honours():
    assert HONOURED in rej.ATTN and len([n for n in rej.ATTN if n != HONOURED]) == 16 and rej.EXACT in rej.ATTN


def test_the_honoured_entry_refuses_the_flag_without_causal_and_with_single_accumulation():
    rc, err = _call(HONOURED, _cabi.ATTR_CAUSAL_BOTTOM_RIGHT, is_causal=0)
    assert rc == -1 and FLAG in err and b"is_causal = 1" in err, (rc, err)
    rc, err = _call(HONOURED, _cabi.ATTR_CAUSAL_BOTTOM_RIGHT, is_causal=1, pv_accum=_cabi.PV_ACCUM_SINGLE)
    assert rc == -1 and FLAG in err and b"SAGE_PV_ACCUM_TWO_LEVEL" in err, (rc, err)


def test_the_honoured_entry_takes_the_flag_as_far_as_the_checks_go():
    """Causal and two-level: the next refusal is the one asked for (head_dim 96), not the flag's -- the tensors are host memory."""
    for flags in (_cabi.ATTR_CAUSAL_BOTTOM_RIGHT, _cabi.ATTR_CAUSAL_BOTTOM_RIGHT | _cabi.ATTR_FP8_EXACT_SCORES):
        rc, err = _call(HONOURED, flags, is_causal=1, D=96)
        assert rc == -1 and b"head_dim must be 64 or 128 (got 96)" in err and FLAG not in err, (rc, err)


@pytest.mark.parametrize("name", rej.ATTN)
@pytest.mark.parametrize("bit", [0x10, 0x20, 0x40])
def test_the_bits_above_stay_unknown(name, bit):
    for flags in (bit, bit | _cabi.ATTR_CAUSAL_BOTTOM_RIGHT):
        rc, err = _call(name, flags, **({} if name.endswith("_masked") else dict(is_causal=1)))
        assert rc == -1 and b"unknown SageLaunchAttr.flags" in err, (rc, err)


def test_launch_attr_carries_the_flag():
    assert _cabi.launch_attr() is None and _cabi.launch_attr(causal_bottom_right=False) is None
    a = _cabi.launch_attr(causal_bottom_right=True)
    assert a is not None and a.flags == 8 and a.struct_bytes == 56 and a.window == 0 and not a.q_start and not a.launch_ws
    a = _cabi.launch_attr(causal_bottom_right=True, folded_scores=True)
    assert a.flags == 8 | 4
    assert _cabi.launch_attr(window=5).flags == 0
    from sageattention_amd import ops
    assert "causal_bottom_right" in inspect.signature(ops.attn_attr).parameters
    assert inspect.signature(ops.attn_attr).parameters["causal_bottom_right"].default is False


# ---------------------------------------------------------------------------------------------- the work list
def _items(lq, lk, mode, hq=8, hkv=2, D=128):
    lib = _cabi.load()
    lq, lk = np.ascontiguousarray(lq, np.int32), np.ascontiguousarray(lk, np.int32)
    cap = int(((lq + 127) // 128).sum()) + 1
    out, hdr = np.zeros((cap, 2), np.int32), np.zeros(8, np.int32)
    grid = lib.sage_debug_varlen_items(lq.ctypes.data_as(ctypes.c_void_p), lk.ctypes.data_as(ctypes.c_void_p), len(lq), mode, hq, hkv, D, 1,
                                       out.ctypes.data_as(ctypes.c_void_p), cap, hdr.ctypes.data_as(ctypes.c_void_p))
    assert grid >= 0, lib.sage_last_error()
    assert hdr[0] == cap - 1
    return [tuple(r) for r in out[:hdr[0]].tolist()], hdr[:4].tolist(), grid


def _length_sets():
    """200 seeded sets, nseq 1 .. 40: free lengths, Lq > Lk, zero lengths on either side, Lq = Lk, and every tenth set Lq = Lk throughout."""
    rng = np.random.default_rng(20)
    for t in range(200):
        n = int(rng.integers(1, 41))
        lq, lk = rng.integers(0, 1500, n), rng.integers(0, 3000, n)
        m = rng.random(n)
        lk = np.where(m < 0.2, lq, lk)                          # Lq = Lk
        lk = np.where((m >= 0.2) & (m < 0.4), lq // 3, lk)      # Lq > Lk: blocks wholly in front of key 0
        lk = np.where((m >= 0.8) & (m < 0.9), 0, lk)            # no keys
        lq = np.where(m >= 0.9, 0, lq)                          # no rows
        if t % 10 == 0:
            lk = lq.copy()
        yield t, lq.astype(np.int32), lk.astype(np.int32)


def test_the_bottom_right_work_list_is_the_brute_force_sort():
    seen_zero = seen_gt = 0
    for t, lq, lk in _length_sets():
        blocks = [(s, j) for s in range(len(lq)) for j in range((int(lq[s]) + 127) // 128)]
        want = sorted(blocks, key=lambda x: (-rb.item_weight(int(lq[x[0]]), int(lk[x[0]]), x[1]), x[0], -x[1]))
        got, hdr, grid = _items(lq, lk, 2)
        assert sorted(got) == blocks, t                                    # a permutation of the blocks that exist
        assert got == want, t
        seen_zero += sum(rb.item_weight(int(lq[s]), int(lk[s]), j) == 0 and lk[s] > 0 for s, j in blocks)
        seen_gt += int((lq > lk).sum())
        if got:                                                           # weight 0 stays in the list, last
            ws = [rb.item_weight(int(lq[s]), int(lk[s]), j) for s, j in got]
            assert ws == sorted(ws, reverse=True)
        one, hdr1, grid1 = _items(lq, lk, 1)
        assert sorted(one) == blocks and hdr1 == hdr and grid1 == grid    # (the plan over the list does not depend on the weights)
        if t % 10 == 0:
            assert got == one, t                                          # Lq = Lk throughout: the top-left list
    assert seen_zero > 50 and seen_gt > 200                               # (the draws did reach blocks in front of key 0)


def test_other_causal_values_keep_their_meaning():
    rng = np.random.default_rng(21)
    lq, lk = rng.integers(0, 2000, 30).astype(np.int32), rng.integers(0, 2000, 30).astype(np.int32)
    assert _items(lq, lk, 1) == _items(lq, lk, 3) == _items(lq, lk, -1)      # any non-zero value but 2: top-left
    assert _items(lq, lk, 0)[0] != _items(lq, lk, 1)[0] != _items(lq, lk, 2)[0]
    top = sorted([(s, j) for s in range(30) for j in range((int(lq[s]) + 127) // 128)],
                 key=lambda x: (-min(2 * x[1] + 2, (int(lk[x[0]]) + 63) // 64), x[0], -x[1]))
    assert _items(lq, lk, 1)[0] == top


def test_the_weight_is_the_kernels_tile_count_and_monotone():
    rng = np.random.default_rng(22)
    for _ in range(3000):
        lq, lk = int(rng.integers(1, 3000)), int(rng.integers(0, 3000))
        ws = [rb.item_weight(lq, lk, j) for j in range((lq + 127) // 128)]
        assert ws == [rb.loop_bounds(lq, lk, j)["n_iters"] for j in range(len(ws))]
        assert ws == sorted(ws)


# ---------------------------------------------------------------------------------------------- the loop bounds against the predicate
def test_loop_bounds_cover_the_predicate():
    """20 000 seeded (Lq, Lk, query block): every visible key lies in a tile that runs; the unmasked (steady) tiles are whole and wholly visible
    to every row of the block; when the pipelined last-tile bodies run (diag_ok), the two tiles they take are whole and every row of the
    block sees key 0 -- a masked score there still sets a row maximum, which only a row with a visible key may have."""
    rng = np.random.default_rng(23)
    n_diag = n_front = n_three = 0
    for t in range(20000):
        kind = t % 4
        lq = int(rng.integers(1, 1200))
        lk = int(rng.integers(0, 2400))
        if kind == 1:
            lk = max(0, lq + 64 * int(rng.integers(-6, 30)))        # offsets that are multiples of 64
        elif kind == 2:
            lq, lk = int(rng.integers(1, 40)), int(rng.integers(0, 1500))      # decode / verification rows
        elif kind == 3:
            lk = int(rng.integers(0, lq + 1))                       # more rows than keys
        qblk = int(rng.integers(0, (lq + 127) // 128))
        s = lk - lq
        b = rb.loop_bounds(lq, lk, qblk)
        assert b["kchunk0"] == -s and 0 <= b["n_iters"] <= (lk + 63) // 64
        r0, r1 = 128 * qblk, min(lq, 128 * qblk + 128)              # the rows of the block that exist
        last_visible = min(lk - 1, r1 - 1 + s)                      # of the block's last row: the largest of all
        if last_visible >= 0:
            assert last_visible // 64 < b["n_iters"], (lq, lk, qblk, b)
        else:
            n_front += 1
        assert b["n_iters"] == 0 or 64 * (b["n_iters"] - 1) <= 128 * qblk + 127 + s      # (no tile wholly behind the block's diagonal runs)
        ns = max(b["n_steady"], 0)
        if ns:
            # whole tiles, and their last key visible to the block's FIRST row -- hence to all 128 rows of the block, those past Lq included
            assert 64 * ns <= lk and 64 * ns - 1 <= r0 + s, (lq, lk, qblk, b)
            assert ns + 2 <= b["n_iters"]                           # (the pipelined loop looks two tiles ahead)
        if b["diag_ok"]:
            n_diag += 1
            assert s % 64 == 0 and b["n_iters"] - ns == 2 and 64 * b["n_iters"] <= lk, (lq, lk, qblk, b)
            assert r0 + s >= 0, (lq, lk, qblk, b)                   # every row of the block sees key 0
        elif b["n_iters"] - ns == 3:
            n_three += 1
    assert n_diag > 500 and n_front > 500 and n_three > 500


def test_loop_bounds_of_the_tested_batch():
    """The shapes of tests/test_gpu_varlen_br.py's batch reach what its table says."""
    b = rb.loop_bounds(200, 640, 0)
    assert (b["n_iters"], b["n_steady"], b["diag_ok"]) == (9, 6, False)             # offset 440: three general tiles behind six steady ones
    b = rb.loop_bounds(200, 640, 1)
    assert (b["n_iters"], b["n_steady"], b["diag_ok"]) == (10, 8, False)            # ... and the second block: cut by the last key, two general tiles
    b = rb.loop_bounds(128, 512, 0)
    assert (b["n_iters"], b["n_steady"], b["diag_ok"]) == (8, 6, True)              # offset 384: the pipelined diagonal
    assert rb.loop_bounds(1, 300, 0)["n_iters"] == 5 and rb.loop_bounds(16, 1000, 0)["n_iters"] == 16
    assert [rb.loop_bounds(300, 130, j)["n_iters"] for j in range(3)] == [0, 2, 3] and rb.rows_without_keys(300, 130) == 170
    assert [rb.loop_bounds(260, 1, j)["n_iters"] for j in range(3)] == [0, 0, 1] and rb.rows_without_keys(260, 1) == 259
    assert rb.loop_bounds(70, 0, 0)["n_iters"] == 0 and rb.rows_without_keys(70, 0) == 70
    assert rb.loop_bounds(129, 129, 1)["n_iters"] == 3 and rb.loop_bounds(5, 64, 0)["n_iters"] == 1
    for lq, lk in ((200, 640), (300, 130), (260, 1), (5, 64), (1, 300)):
        keep = rb.visible(lq, lk)
        assert int((~keep.any(axis=1)).sum()) == rb.rows_without_keys(lq, lk)
        for i in (0, lq // 2, lq - 1):
            assert np.flatnonzero(keep[i]).tolist() == [j for j in range(lk) if j <= i + lk - lq]


# ---------------------------------------------------------------------------------------------- the build
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_packed_br_units_build_within_the_family_targets():
    """The units are in the Makefile's SRCS; each holds the causal two-level exact-score kernel for fp16 and bf16 q (QF 3 / 4), with and
    without the ticket loop (CPERS): four kernels per unit, zero scratch, D = 128 at two waves per SIMD, D = 64 at three."""
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
        forms = {name: tbr.kf.decode(name) for name in mine}
        for name, res in mine.items():
            # D, FP8 PV, causal, per-block k scales, two-level, no mask, the exact form ... no WINDOW, QSTART, no KVLEN; QF 3 / 4 and CPERS or not
            f = forms[name]
            assert f == tbr.kf.form(128 if d128 else 64, pv_fp8=True, causal=True, two_level=True, qstart=True, qf=f["qf"], cpers=f["cpers"]), name
            assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0, (name, res)
            assert res["Occupancy"] >= (2 if d128 else 3) and res["VGPRs"] <= (256 if d128 else 168), (name, res)
        # QF 3 and 4 (fp16, bf16), the exact score form, each with CPERS and without
        assert {(f["qf"] == 3, f["cpers"]) for f in forms.values()} == {(a, b) for a in (True, False) for b in (True, False)}, sorted(mine)
        assert all((f["qf"] == 3) != (f["qf"] == 4) for f in forms.values()), sorted(mine)


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_packed_br_units_pass_the_mfma_hazard_lint():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_hazard_lint as lint
    assert lint.UNITS_PACKED_BR == UNITS and not set(UNITS) & set(lint.UNITS + lint.UNITS_PAIR + lint.UNITS_WINDOW)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as ex:
        results = dict(zip(UNITS, ex.map(lambda u: lint.lint(lint.listing(u)), UNITS)))
    for unit, (findings, n_mfma) in results.items():
        assert n_mfma >= 200, (unit, n_mfma)                   # (four kernels: the walk did see the pipelined loops)
        assert not findings, (unit, findings[:5])
