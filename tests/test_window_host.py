"""CPU: the sliding window of the FP8-PV route (``window_size=``) -- the definition (the predicate of the kernel's parameters against the one
of the public keywords, the rows that see nothing against a closed form), the predicate restatement ``tests/ref_window.py`` pinned to the C
oracle's causal path, the keyword's argument errors, the ``window`` field of ``SageLaunchAttr`` (the struct's former ``reserved`` word: which
entry point takes it, that zero and a shorter struct change nothing), and the build of the kernels behind the route (units
sage_attn_d{128,64}_f8w.hip: instantiation count, zero scratch, the family's occupancy, the MFMA hazard lint)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import util
import ref_window as rw
import test_build_resources as tbr
import test_cabi_attn_rejects as rej
from sageattention_amd import _cabi, core as sc, processors
from test_cabi import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("sage_attn_d128_f8w.hip", "sage_attn_d64_f8w.hip")
LK, LQ = rw.LK, rw.LQ


def _cpu_qkv(B=2, Lk=256, D=64):
    z = lambda L: torch.zeros(B, 2, L, D, dtype=torch.float16)
    return z(16), z(Lk), z(Lk)


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("length,s,W", rw.WINDOW_CASES)
def test_the_parameters_and_the_keywords_describe_one_predicate(length, s, W):
    keep = rw.visible(LQ, LK, s, W, 0, length)
    assert torch.equal(keep, rw.visible_from_keywords(LQ, LK, (W - 1, 0), True, s, length))
    assert torch.equal(keep, rw.visible_from_keywords(LQ, LK, (W - 1, -1), True, s, length))
    assert torch.equal(keep, rw.visible_from_keywords(LQ, LK, (W - 1, 0), False, s, length))          # (right = 0 without is_causal: the same rows and keys)
    assert sc._window_args((W - 1, 0), True, "per_thread", "fp32+fp16", False, {}) == (W, 0)
    assert sc._window_args((W - 1, 0), False, "per_thread", "fp32+fp16", False, {}) == (W, 0)
    assert int((~keep.any(dim=1)).sum()) == rw.rows_without_keys(LQ, s, W, length)
    # brute force, key by key
    for i in (0, 1, 48, 49, 127, 128, LQ - 1):
        want = [j for j in range(LK) if s + i - W < j <= s + i and 0 <= j < length]
        assert torch.nonzero(keep[i]).flatten().tolist() == want, i


@pytest.mark.parametrize("ws,W,r", [((100, 30), 131, 30), ((-1, 30), 0, 30), ((63, 0), 64, 0), ((0, 0), 1, 0), ((5, 200), 206, 200)])
def test_a_non_causal_window_is_a_shifted_causal_one(ws, W, r):
    assert sc._window_args(ws, False, "per_thread", "fp32+fp16", False, {}) == (W, r)
    for length, s in ((640, 0), (577, 377), (130, -70)):
        assert torch.equal(rw.visible(LQ, LK, s, W, r, length), rw.visible_from_keywords(LQ, LK, ws, False, s, length)), (length, s)


def test_unbounded_windows_are_no_window_and_the_window_is_capped():
    for ws, causal in ((None, True), (None, False), ((-1, -1), True), ((-1, -1), False), ((-1, 0), True)):
        assert sc._window_args(ws, causal, "per_thread", "fp32+fp16", False, {}) is None
    assert sc._window_args((2 ** 30 - 1, 0), True, "per_thread", "fp32+fp16", False, {}) == (2 ** 30, 0)
    assert sc._window_args((2 ** 40, 0), True, "per_thread", "fp32+fp16", False, {}) == (2 ** 30, 0)


# ---------------------------------------------------------------------------------------------- the restatement against the oracle
def _mk(shape, dtype, seed, bias=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if bias:
        x = x + bias * torch.randn(shape[:-2] + (1, shape[-1]), generator=g)
    return x.to(dtype)


@pytest.mark.parametrize("D,dtype", [(64, torch.float16), (64, torch.bfloat16), (128, torch.float16), (128, torch.bfloat16)])
def test_the_restatement_is_the_oracles_causal_path(oracle_mod, D, dtype):
    """Predicates the oracle can express -- causal, and causal shifted by an offset (zero rows in front of q8 for a positive offset, rows
    dropped for a negative one, as test_gpu_q_start.py::_oracle_sample restates it) -- under test_second_restatement.py's criterion: o within
    one output ulp on fewer than 2e-3 of the elements, lse within 2e-6 max(1, max|lse|).  The measured share is printed."""
    oracle = oracle_mod
    code = oracle.F16 if dtype == torch.float16 else oracle.BF16
    Hq, Hkv = 2, 1
    q, k, v = _mk((1, Hq, LQ, D), dtype, 1), _mk((1, Hkv, LK, D), dtype, 2, bias=3.0), _mk((1, Hkv, LK, D), dtype, 3)
    for length, s in ((640, 0), (577, 377), (130, -70)):
        kb, vb = k[:, :, :length].contiguous(), v[:, :, :length].contiguous()
        _, _, aux = oracle.sageattn_dense(util.bits(q), util.bits(kb), util.bits(vb), code, is_causal=True, pv="f8", qk_quant_gran="per_thread",
                                          return_lse=True, smooth_k=True, fp8_scores="exact")
        q8, gq = aux["q8"], aux["gq"]
        front, drop = max(0, s), max(0, -s)
        q8s = np.ascontiguousarray(np.concatenate([np.zeros(q8.shape[:2] + (front, D), np.int8), q8[:, :, drop:]], axis=2))
        gqs = np.concatenate([np.zeros(front, np.int32), gq[drop:]])
        o_c, lse_c = oracle.attn(q8s, aux["k8"], aux["v8"], aux["qs"], gqs, aux["ks"], aux["gk"], causal=True, c=aux["c"],
                                 pv_mode=oracle.PV_F8_TWO_LEVEL, out_dtype=code, v_scale=aux["vs"], return_lse=True, score_mode=oracle.SCORES_EXACT)
        o_w, lse_w = rw.attn_window(q8[0], aux["k8"][0], aux["v8"][0], aux["qs"][0], gq, aux["ks"][0], aux["gk"], aux["vs"][0],
                                    rw.visible(LQ, length, s, 0, 0, length), c=np.float32(aux["c"]), out_dtype=dtype)
        empty = torch.isneginf(lse_w)
        assert int(empty.sum()) == Hq * rw.rows_without_keys(LQ, s, 0, length) == Hq * drop
        assert not o_w[empty].float().abs().sum() and not torch.signbit(o_w[empty].float()).any()
        got, want = util.bits(o_w)[:, drop:].astype(np.int32), o_c[0, :, front:].astype(np.int32)
        diff = np.abs(got - want)
        lerr = float(np.abs(lse_w.numpy()[:, drop:] - lse_c[0, :, front:]).max())
        print(f"D {D} {dtype} len {length} offset {s}: {float((diff != 0).mean()):.2e} of the outputs differ (max {int(diff.max())} ulp), lse {lerr:.2e}")
        assert diff.max() <= 1 and (diff != 0).mean() < 2e-3, (length, s, int(diff.max()), float((diff != 0).mean()))
        assert lerr <= 2e-6 * max(1.0, float(np.abs(lse_c[0, :, front:]).max())), (length, s, lerr)


# ---------------------------------------------------------------------------------------------- Python: argument errors
@pytest.mark.parametrize("causal,ws", [(True, (63, 0)), (False, (100, 30)), (False, (-1, 30))], ids=["causal", "non_causal", "unbounded_left"])
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
def test_refused_options_name_themselves_and_the_keyword(causal, ws, kw, msg):
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match=msg) as e:
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=causal, window_size=ws, **kw)
    assert "window_size" in str(e.value)


@pytest.mark.parametrize("causal,ws", [(True, (63, 1)), (True, (63, 30)), (True, (-1, 5)), (True, (-2, 0)), (False, (63, -2)), (False, (-5, -5)),
                                       (False, (63, -1)), (True, (63.0, 0)), (True, (True, 0)), (True, 63), (True, (63,)), (True, (63, 0, 0)),
                                       (True, "63"), (True, (torch.tensor(63), 0)), (False, (None, 0))])
def test_a_bad_window_raises(causal, ws):
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match="window_size"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=causal, window_size=ws)


@pytest.mark.parametrize("causal,ws", [(True, (63, 0)), (True, (63, -1)), (True, (0, 0)), (False, (100, 30)), (False, (-1, 30)), (False, (63, 0)),
                                       (True, (-1, -1)), (True, [63, 0])])
@pytest.mark.parametrize("kw", [dict(), dict(split_kv=None), dict(split_kv=0), dict(pv_accum_dtype="fp32+fp32"), dict(smooth_k=False),
                                dict(kv_lens=torch.full((2,), 100, dtype=torch.int32)), dict(q_start=torch.full((2,), 100, dtype=torch.int32)),
                                dict(q_start=7), dict(causal_align="bottom_right")],
                         ids=["default", "split_none", "split_0", "fp32+fp32", "nosk", "kv_lens", "q_start", "q_start_int", "bottom_right"])
def test_supported_options_pass_the_argument_check(causal, ws, kw):
    q, k, v = _cpu_qkv()
    with pytest.raises(AssertionError, match="cuda"):        # (accepted; then the ordinary input check of a CPU tensor)
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=causal, window_size=ws, **kw)


def test_torch_compile_refuses_the_keyword(monkeypatch):
    q, k, v = _cpu_qkv()
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    for fn in (sc.sageattn_qk_int8_pv_fp8_cuda, sc.sageattn, processors.sdpa):
        with pytest.raises(ValueError, match="window_size is not supported under torch.compile"):
            fn(q, k, v, is_causal=True, window_size=(63, 0))


def test_sdpa_takes_a_mask_or_a_window_and_the_mirror_package_has_the_keyword():
    import sageattention
    q, k, v = _cpu_qkv()
    for causal, ws in ((True, (63, 0)), (False, (63, 30))):
        with pytest.raises(ValueError, match="attn_mask or window_size"):
            processors.sdpa(q, k, v, attn_mask=torch.ones(16, 256, dtype=torch.bool), is_causal=causal, window_size=ws)
    for fn in (sageattention.sageattn, sageattention.sageattn_qk_int8_pv_fp8_cuda, sc.sageattn, processors.sdpa):
        assert "window_size" in inspect.signature(fn).parameters, fn
    assert sageattention.sageattn_qk_int8_pv_fp8_cuda is sc.sageattn_qk_int8_pv_fp8_cuda


def test_right_is_folded_into_the_offsets_without_a_host_read():
    """The diagonal's shift is added by tensor ops on the offsets' device (a meta tensor has no data to read), saturating at int32's end."""
    lens = torch.empty(3, dtype=torch.int64, device="meta")
    for args in ((None, lens), (torch.empty(3, dtype=torch.int64, device="meta"), None), (torch.empty(3, dtype=torch.int32, device="meta"), lens)):
        s = sc._q_start_tensor(*args, 3, 200, 640, lens.device, 30)
        assert s.device.type == "meta" and s.dtype == torch.int32 and s.shape == (3,)
    assert sc._q_start_tensor(0, None, 2, 200, 640, "cpu", 30).tolist() == [30, 30]
    assert sc._q_start_tensor(None, torch.tensor([700, 640, 100, 0, -4]), 5, 200, 640, "cpu", 30).tolist() == [470, 470, -70, -170, -170]
    assert sc._q_start_tensor(torch.tensor([2 ** 40, -2 ** 40, 5]), None, 3, 200, 640, "cpu", 30).tolist() == [2 ** 31 - 1, -2 ** 31 + 30, 35]
    assert sc._q_start_tensor(torch.tensor([5, 6], dtype=torch.int32), None, 2, 200, 640, "cpu", 0).tolist() == [5, 6]


# ---------------------------------------------------------------------------------------------- C ABI
def test_the_field_takes_the_reserved_word_and_the_abi_is_unchanged():
    lib = _cabi.load()
    header = open(os.path.join(ROOT, "include", "sage_gfx950.h")).read()
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22 and len(prototypes()) == 56 and len(_cabi.SYMBOLS) == 56
    body = re.search(r"typedef struct SageLaunchAttr \{(.*?)\} SageLaunchAttr;", header, re.S).group(1)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert fields[-2:] == ["int32_t window", "const int32_t *q_start"] and "reserved" not in body
    names = [f[0] for f in _cabi.SageLaunchAttr._fields_]
    assert names[-2:] == ["window", "q_start"] and "reserved" not in names
    assert _cabi.SageLaunchAttr.window.offset == 44 and _cabi.SageLaunchAttr.q_start.offset == 48 and ctypes.sizeof(_cabi.SageLaunchAttr) == 56
    assert re.search(r"^ \*  window\s", header, re.M), "the header's attribute block documents the field"


def _call(name, attr, **wrong):
    """``name`` with the refusal table's valid arguments (host memory: the library must refuse before its first HIP call) but for ``wrong``."""
    args = []
    for ctype, pname in prototypes()[name][1]:
        args.append(wrong[pname] if pname in wrong else rej.VALID[pname] if pname in rej.VALID else rej.P)
    args[-1] = ctypes.byref(attr) if attr is not None else None
    lib = _cabi.load()
    return getattr(lib, name)(*args), lib.sage_last_error()


def _attr(window=64, q_start=None, flags=0, struct_bytes=None):
    a = _cabi.SageLaunchAttr()
    a.struct_bytes = ctypes.sizeof(a) if struct_bytes is None else struct_bytes
    a.flags = flags
    a.window = window
    a.q_start = q_start
    return a


@pytest.mark.parametrize("name", [n for n in rej.ATTN if n != rej.KVLENS])
@pytest.mark.parametrize("causal", [0, 1])
def test_every_other_entry_point_refuses_a_window(name, causal):
    rc, err = _call(name, _attr(), **({} if name.endswith("_masked") else dict(is_causal=causal)))
    assert rc == -1 and b"SageLaunchAttr.window" in err, (rc, err)


def test_the_kvlens_entry_refuses_a_window_without_causal_and_with_folded_scores():
    rc, err = _call(rej.KVLENS, _attr(), is_causal=0)
    assert rc == -1 and b"SageLaunchAttr.window" in err and b"is_causal = 1" in err, (rc, err)
    rc, err = _call(rej.KVLENS, _attr(flags=_cabi.ATTR_FP8_FOLDED_SCORES), is_causal=1)
    assert rc == -1 and b"window" in err, (rc, err)
    # causal and exact, with offsets and without: accepted as far as the checks go (the next refusal is the one asked for, not the window's)
    for qs in (None, rej.P):
        rc, err = _call(rej.KVLENS, _attr(q_start=qs), is_causal=1, D=96)
        assert rc == -1 and b"head_dim" in err and b"window" not in err, (rc, err)


@pytest.mark.parametrize("name", rej.ATTN)
def test_a_negative_window_is_refused(name):
    for w in (-1, -2 ** 31):
        rc, err = _call(name, _attr(window=w), **({} if name.endswith("_masked") else dict(is_causal=1)))
        assert rc == -1 and b"SageLaunchAttr.window" in err and str(w).encode() in err, (rc, err)


@pytest.mark.parametrize("name", rej.ATTN)
def test_a_zero_window_and_an_older_struct_change_nothing(name):
    """A struct that ends before the field (40 bytes) or at it (44) is read as far as it goes: what lies behind -- here a window, even a
    negative one -- is not seen.  The call goes on to the refusal asked for (head_dim 96): the tensors are host memory."""
    for attr in (_attr(window=0), _attr(struct_bytes=40), _attr(struct_bytes=44), _attr(window=-7, struct_bytes=44), _attr(struct_bytes=46),
                 _attr(struct_bytes=8)):
        rc, err = _call(name, attr, D=96)
        assert rc == -1 and b"head_dim must be 64 or 128 (got 96)" in err, (rc, err)


def test_launch_attr_carries_the_window():
    assert _cabi.launch_attr() is None and _cabi.launch_attr(window=0) is None
    a = _cabi.launch_attr(window=1024)
    assert a is not None and a.window == 1024 and not a.q_start and a.struct_bytes == 56 and a.flags == 0 and not a.launch_ws
    assert bytes(a)[44:48] == (1024).to_bytes(4, "little")
    t = torch.zeros(4, dtype=torch.int32)
    a = _cabi.launch_attr(q_start=t, window=7)
    assert a.window == 7 and a.q_start == t.data_ptr()
    assert _cabi.launch_attr(q_start=t).window == 0


# ---------------------------------------------------------------------------------------------- the build
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_window_units_build_within_the_family_targets():
    """The units are in the Makefile's SRCS; each holds the causal kernel for fp16 and for bf16 q: four kernels over the two units, with zero
    scratch, D = 128 at two waves per SIMD, D = 64 at three."""
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
            # D, FP8 PV, causal, per-thread, two-level, the exact form ... WINDOW, QSTART, KVLEN and nothing else
            assert forms[name] == tbr.kf.form(128 if d128 else 64, pv_fp8=True, causal=True, kthread=True, two_level=True, window=True, qstart=True,
                                              kvlen=True, qf=forms[name]["qf"]), name
            assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0, (name, res)
            assert res["Occupancy"] >= (2 if d128 else 3) and res["VGPRs"] <= (256 if d128 else 168), (name, res)
        assert {f["qf"] for f in forms.values()} == {1, 2}, sorted(mine)      # (QF 1 and 2: fp16, bf16)


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_window_units_pass_the_mfma_hazard_lint():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_hazard_lint as lint
    assert lint.UNITS_WINDOW == UNITS and not set(UNITS) & set(lint.UNITS + lint.UNITS_PAIR)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as ex:
        results = dict(zip(UNITS, ex.map(lambda u: lint.lint(lint.listing(u)), UNITS)))
    for unit, (findings, n_mfma) in results.items():
        assert n_mfma >= 100, (unit, n_mfma)                   # (two kernels: the walk did see the pipelined loops)
        assert not findings, (unit, findings[:5])
