"""CPU: the sliding window of the packed FP8-PV route (``sageattn_qk_int8_pv_fp8_varlen(causal_align="bottom_right", window_size=...)``) --
the definition (the predicate of (Lq, Lk, W) against FlashAttention's (left, right) form, the rows that see nothing), the restatement
``tests/ref_varlen_window.py`` pinned to the C oracle's packed causal path, the keyword's argument errors, the C ABI rule (the packed entry
honours ``SageLaunchAttr.window`` only together with SAGE_ATTR_CAUSAL_BOTTOM_RIGHT; nothing else changes), the kernel's loop bounds restated
in Python against the predicate, and the build of the kernels behind the route (units sage_attn_d{128,64}_f8vbw.hip)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import util
import ref_varlen_br as rb
import ref_varlen_window as rvw
import test_build_resources as tbr
import test_cabi_attn_rejects as rej
from sageattention_amd import _cabi, core as sc
from test_cabi import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("sage_attn_d128_f8vbw.hip", "sage_attn_d64_f8vbw.hip")
PACKED = "sage_attn_fused_qblock_pv_f8_varlen"
BR = _cabi.ATTR_CAUSAL_BOTTOM_RIGHT
# the batch of tests/test_gpu_varlen_window.py
BATCH = ((448, 448), (128, 568), (128, 1024), (1, 1000), (1, 50), (5, 700), (300, 130), (7, 1), (64, 0), (0, 200), (128, 128))
WINDOWS = (1, 100, 192, 448)


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("lq,lk", [(40, 90), (90, 40), (1, 70), (33, 33), (5, 0), (0, 9), (70, 1)])
@pytest.mark.parametrize("W", [1, 2, 17, 64, 200])
def test_the_parameters_and_the_keywords_describe_one_predicate(lq, lk, W):
    keep = rvw.visible(lq, lk, W)
    assert np.array_equal(keep, rvw.visible_from_keywords(lq, lk, (W - 1, 0)))
    assert np.array_equal(keep, rvw.visible_from_keywords(lq, lk, (W - 1, -1)))
    assert np.array_equal(rvw.visible(lq, lk, 0), rvw.visible_from_keywords(lq, lk, (-1, 0)))
    assert np.array_equal(rvw.visible(lq, lk, 0), rb.visible(lq, lk))
    s = lk - lq
    for i in range(lq):                                                    # the issue's sentence, key by key
        assert np.flatnonzero(keep[i]).tolist() == [j for j in range(lk) if s + i - W < j <= s + i and 0 <= j < lk], i
    assert int((~keep.any(axis=1)).sum()) == rvw.rows_without_keys(lq, lk, W) == rb.rows_without_keys(lq, lk)
    assert sc._varlen_window_args((W - 1, 0), True, "bottom_right", "fp32+fp32", lq, lk, {}) == W


def test_unbounded_windows_are_no_window_and_the_window_is_capped():
    for ws, causal in ((None, True), (None, False), ((-1, -1), True), ((-1, -1), False), ((-1, 0), True)):
        for align in ("top_left", "bottom_right"):
            assert sc._varlen_window_args(ws, causal, align, "fp32", 10, 10, dict(fuse_q_quant=False)) == 0
    assert sc._varlen_window_args((2 ** 30 - 1, 0), True, "bottom_right", "fp32+fp32", 10, 10, {}) == 2 ** 30
    assert sc._varlen_window_args((2 ** 40, -1), True, "bottom_right", "fp32+fp32", 10, 10, {}) == 2 ** 30
    w = sc._varlen_window_args([0, 0], True, "bottom_right", "fp32+fp32", 10, 10, {})
    assert w == 1 and type(w) is int


# ---------------------------------------------------------------------------------------------- the restatement against the oracle
def _mk(pairs, Hq, Hkv, D, dtype, seed):
    lq, lk = [p[0] for p in pairs], [p[1] for p in pairs]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(sum(lq), Hq, D, generator=g).to(dtype)
    k = (torch.randn(sum(lk), Hkv, D, generator=g) + torch.randn(1, Hkv, D, generator=g)).to(dtype)
    v = torch.randn(sum(lk), Hkv, D, generator=g).to(dtype)
    cu = lambda x: np.concatenate([[0], np.cumsum(x)]).astype(np.int32)
    return util.bits(q), util.bits(k), util.bits(v), cu(lq), cu(lk)


def _oracle_top_left(O, q, k, v, dt, cu_q, cu_k):
    """The oracle's causal path (top-left) on the packed FP8 route's operands, per sequence; K as given (no smoothing, no lse correction)."""
    Hq, D = q.shape[1], q.shape[2]
    o, lse = np.zeros(q.shape, np.uint16), np.full((Hq, q.shape[0]), -np.inf, np.float32)
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        lq, lk = q1 - q0, k1 - k0
        t = lambda x, a, e: np.ascontiguousarray(x[a:e].transpose(1, 0, 2))[None]
        gq, nq = O.group_index(lq, "per_block", "q", 128, 128)
        gk, nk = O.group_index(lk, "per_block", "k", 64, 64)
        q8, qsc = O.quant_int8(t(q, q0, q1), dt, gq, nq, pre_scale=np.float32(O.LOG2E / D ** 0.5), style=O.STYLE_TRITON)
        k8, ksc = O.quant_int8(t(k, k0, k1), dt, gk, nk, style=O.STYLE_TRITON)
        v8, vs = O.quant_v_fp8(t(v, k0, k1), dt)
        ob, lb = O.attn(q8, k8, v8, qsc, gq, ksc, gk, causal=True, c=1.0, pv_mode=O.PV_F8_TWO_LEVEL, out_dtype=dt, v_scale=vs, return_lse=True,
                        score_mode=O.SCORES_EXACT)
        o[q0:q1], lse[:, q0:q1] = ob[0].transpose(1, 0, 2), lb[0]
    return o, lse / np.float32(O.LOG2E)


@pytest.mark.parametrize("D,dt", [(64, 0), (64, 1), (128, 0), (128, 1)])
def test_the_restatement_is_the_oracles_packed_causal_path(oracle_mod, D, dt):
    """Predicates the oracle can express: top-left (row i sees keys j <= i; sequences with at least as many keys as rows, so that every row
    sees a key), and bottom-right, the shift restated by padding q8 (tests/ref_varlen_br.py; sequences with more rows than keys, one key and
    no keys included).  The criterion of tests/test_window_host.py: o within one output ulp on at most 2e-3 of the elements, lse within
    2e-6 max(1, max|lse|); rows without keys +0 / -inf on both sides.  The measured share is printed."""
    O = oracle_mod
    Hq, Hkv = 4, 2
    # bottom-right
    pairs = ((200, 328), (128, 512), (1, 300), (16, 200), (300, 130), (70, 1), (9, 0), (129, 129))
    q, k, v, cu_q, cu_k = _mk(pairs, Hq, Hkv, D, torch.float16 if dt == 0 else torch.bfloat16, 100 + D + dt)
    km = O.k_mean(np.ascontiguousarray(k.transpose(1, 0, 2))[None], dt)
    for W in (0, 2 ** 30):
        o_r, l_r = rvw.ref_f8_varlen_window(O, q, k, v, dt, cu_q, cu_k, W, km=km, return_lse=True)
        o_c, l_c = rb.oracle_f8_varlen_br(O, q, k, v, dt, cu_q, cu_k, km=km, return_lse=True)
        _compare(o_r, l_r, o_c, l_c, f"bottom-right W {W} D {D} dt {dt}")
        empty = np.isneginf(l_r)
        assert int(empty.sum()) == Hq * sum(rb.rows_without_keys(a, b) for a, b in pairs)
        rows = empty.T[:, :, None] & np.ones(D, bool)
        assert not o_r[rows].any()                                         # +0: the bit pattern itself
    # top-left
    pairs = ((200, 328), (128, 128), (1, 300), (129, 130), (64, 64))
    q, k, v, cu_q, cu_k = _mk(pairs, Hq, Hkv, D, torch.float16 if dt == 0 else torch.bfloat16, 200 + D + dt)
    km = O.k_mean(np.ascontiguousarray(k.transpose(1, 0, 2))[None], dt)
    top = lambda lq, lk: np.arange(lk)[None, :] <= np.arange(lq)[:, None]
    ks = O.convert(O.to_f32(k, dt) - O.to_f32(np.asarray(km).reshape(1, Hkv, D), dt), "f16" if dt == 0 else "bf16")      # (smoothed once, for both sides)
    o_r, l_r = rvw.ref_f8_varlen_window(O, q, ks, v, dt, cu_q, cu_k, 0, km=None, return_lse=True, keep_of=top)
    o_c, l_c = _oracle_top_left(O, q, ks, v, dt, cu_q, cu_k)
    _compare(o_r, l_r, o_c, l_c, f"top-left D {D} dt {dt}")


def _compare(o_r, l_r, o_c, l_c, tag):
    assert np.array_equal(np.isneginf(l_r), np.isneginf(l_c)), tag
    diff = np.abs(o_r.view(np.int16).astype(np.int32) - o_c.view(np.int16).astype(np.int32))
    seen = ~np.isneginf(l_c)
    lerr = float(np.abs(l_r[seen] - l_c[seen]).max())
    print(f"{tag}: {float((diff != 0).mean()):.2e} of the outputs differ (max {int(diff.max())} ulp), lse {lerr:.2e}")
    assert diff.max() <= 1 and (diff != 0).mean() <= 2e-3, (tag, int(diff.max()), float((diff != 0).mean()))
    assert lerr <= 2e-6 * max(1.0, float(np.abs(l_c[seen]).max())), (tag, lerr)


# ---------------------------------------------------------------------------------------------- Python: argument errors
def _cpu_packed():
    z = lambda n, h: torch.zeros(n, h, 64, dtype=torch.float16)
    cu_q, cu_k = torch.tensor([0, 16, 48], dtype=torch.int32), torch.tensor([0, 100, 256], dtype=torch.int32)
    return (z(48, 4), z(256, 2), z(256, 2), cu_q, cu_k, 32, 156)


BRK = dict(is_causal=True, causal_align="bottom_right")


@pytest.mark.parametrize("kw,msg", [
    (dict(is_causal=False, causal_align="top_left"), "is_causal"),
    (dict(is_causal=True, causal_align="top_left"), "causal_align"),
    (dict(is_causal=True), "causal_align"),
    (dict(BRK, pv_accum_dtype="fp32"), "pv_accum_dtype"),
    (dict(BRK, fuse_q_quant=False), "fuse_q_quant"),
])
@pytest.mark.parametrize("ws", [(63, 0), (0, -1), [5, 0]])
def test_refused_options_name_themselves_and_the_keyword(ws, kw, msg):
    with pytest.raises(ValueError, match=msg) as e:
        sc.sageattn_qk_int8_pv_fp8_varlen(*_cpu_packed(), window_size=ws, **kw)
    assert "window_size" in str(e.value)


def test_top_left_with_a_window_says_why():
    with pytest.raises(ValueError) as e:
        sc.sageattn_qk_int8_pv_fp8_varlen(*_cpu_packed(), is_causal=True, causal_align="top_left", window_size=(63, 0))
    assert "bottom-right aligned" in str(e.value) and "Lq = Lk" in str(e.value) and "coincide" in str(e.value)


@pytest.mark.parametrize("ws", [(63, 0), (63, 30), (-1, 30), (0, 0)])
def test_a_non_causal_window_is_refused(ws):
    with pytest.raises(ValueError, match="window_size") as e:
        sc.sageattn_qk_int8_pv_fp8_varlen(*_cpu_packed(), is_causal=False, window_size=ws)
    assert "is_causal" in str(e.value)


@pytest.mark.parametrize("causal,ws", [(True, (63, 1)), (True, (63, 30)), (True, (-1, 5)), (True, (-2, 0)), (False, (63, -2)), (False, (-5, -5)),
                                       (False, (63, -1)), (True, (63.0, 0)), (True, (True, 0)), (True, 63), (True, (63,)), (True, (63, 0, 0)),
                                       (True, "63"), (True, (torch.tensor(63), 0)), (False, (None, 0))])
def test_a_bad_window_raises(causal, ws):
    with pytest.raises(ValueError, match="window_size"):
        sc.sageattn_qk_int8_pv_fp8_varlen(*_cpu_packed(), is_causal=causal, causal_align="bottom_right" if causal else "top_left", window_size=ws)


def test_lengths_beyond_the_kernels_int_arithmetic_are_refused():
    a = _cpu_packed()
    with pytest.raises(ValueError, match="window_size"):
        sc.sageattn_qk_int8_pv_fp8_varlen(*a[:5], 2 ** 28, 2 ** 28 + 1, window_size=(63, 0), **BRK)


@pytest.mark.parametrize("kw", [dict(BRK, window_size=(63, 0)), dict(BRK, window_size=(63, -1)), dict(BRK, window_size=(0, 0), smooth_k=False),
                                dict(BRK, window_size=(63, 0), return_lse=True, work_list=False, varlen_plan=False, fused_prepass=False),
                                dict(BRK, window_size=(-1, 0)), dict(BRK, window_size=(-1, -1)), dict(BRK, window_size=None),
                                dict(is_causal=True, window_size=(-1, 0)), dict(is_causal=True, window_size=(-1, -1), pv_accum_dtype="fp32"),
                                dict(is_causal=False, window_size=(-1, -1), fuse_q_quant=False), dict(is_causal=False, window_size=None)])
def test_supported_options_pass_the_argument_check(kw):
    with pytest.raises(AssertionError, match="cuda"):        # (accepted; then the ordinary input check of a CPU tensor)
        sc.sageattn_qk_int8_pv_fp8_varlen(*_cpu_packed(), **kw)


def test_the_keyword_is_read_by_name_before_any_device_call():
    sig = inspect.signature(sc.sageattn_qk_int8_pv_fp8_varlen)
    assert list(sig.parameters)[-1] == "kwargs" and "window_size" not in sig.parameters
    doc = sc.sageattn_qk_int8_pv_fp8_varlen.__doc__
    assert "window_size" in doc and "left + 1" in doc
    src = inspect.getsource(sc.sageattn_qk_int8_pv_fp8_varlen)
    assert src.index('kwargs.pop("window_size"') < src.index("_varlen_prepare(")
    assert "window_size" not in (sc.sageattn_varlen.__doc__ or "")                          # (FP16 PV, the reference's name: unchanged)
    with pytest.raises(Exception) as e:                                                    # (there the keyword stays an unknown route switch)
        sc.sageattn_varlen(*_cpu_packed(), is_causal=True, window_size=(63, 0))
    assert not isinstance(e.value, ValueError) or "window_size" not in str(e.value)


def test_the_attributes_carry_flag_and_window_together():
    from sageattention_amd import ops
    assert inspect.signature(ops.attn_attr).parameters["window"].default == 0
    a = _cabi.launch_attr(causal_bottom_right=True, window=193)
    assert a.flags == 8 and a.window == 193 and a.struct_bytes == 56 and not a.q_start and not a.launch_ws
    src = inspect.getsource(sc._varlen_attend_f8)
    assert src.count("window=st.window") == 2                            # with the work list's ticket block, and alone


# ---------------------------------------------------------------------------------------------- C ABI
def test_the_abi_is_unchanged():
    lib = _cabi.load()
    header = open(os.path.join(ROOT, "include", "sage_gfx950.h")).read()
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22 and len(prototypes()) == 56 and len(_cabi.SYMBOLS) == 56
    assert ctypes.sizeof(_cabi.SageLaunchAttr) == 56 and _cabi.SageLaunchAttr.window.offset == 44
    assert [f[0] for f in _cabi.SageLaunchAttr._fields_][-2:] == ["window", "q_start"]
    assert re.findall(r"^#define\s+SAGE_ATTR_\w+\s+(\d+)u", header, re.M) == ["1", "4", "2", "8"]      # no new flag bit
    block = header[header.index(" *  window  "):header.index("typedef struct SageLaunchAttr")]
    win, bit8 = block.split(" *  flags bit 8")
    assert "ONLY TOGETHER WITH" in win and "SAGE_ATTR_CAUSAL_BOTTOM_RIGHT" in win and PACKED in win       # under `window` ...
    assert "`window`" in bit8 and "sliding window" in bit8                                               # ... and under flags bit 8


def _attr(window=64, flags=0):
    a = _cabi.SageLaunchAttr()
    a.struct_bytes, a.flags, a.window = ctypes.sizeof(a), flags, window
    return a


def _call(name, attr, **wrong):
    """``name`` with the refusal table's valid arguments (host memory: the library must refuse before its first HIP call) but for ``wrong``."""
    args = []
    for ctype, pname in prototypes()[name][1]:
        args.append(wrong[pname] if pname in wrong else rej.VALID[pname] if pname in rej.VALID else rej.P)
    args[-1] = ctypes.byref(attr)
    lib = _cabi.load()
    return getattr(lib, name)(*args), lib.sage_last_error()


@pytest.mark.parametrize("window", [1, 64, 2 ** 30, 2 ** 31 - 1])
def test_the_packed_entry_takes_flag_and_window_as_far_as_the_checks_go(window):
    """Causal, two-level, the flag: the next refusal is the one asked for (head_dim 96), not the window's -- the tensors are host memory."""
    for flags in (BR, BR | _cabi.ATTR_FP8_EXACT_SCORES):
        rc, err = _call(PACKED, _attr(window, flags), is_causal=1, D=96)
        assert rc == -1 and b"head_dim must be 64 or 128 (got 96)" in err and b"window" not in err, (rc, err)


def test_the_packed_entry_refuses_a_window_without_what_it_needs():
    for kw, flags in ((dict(is_causal=1), 0), (dict(is_causal=0), 0), (dict(is_causal=0), BR),
                      (dict(is_causal=1, pv_accum=_cabi.PV_ACCUM_SINGLE), BR), (dict(is_causal=1), _cabi.ATTR_FP8_EXACT_SCORES)):
        rc, err = _call(PACKED, _attr(64, flags), **kw)
        assert rc == -1 and b"SageLaunchAttr.window" in err, (kw, flags, rc, err)
    rc, err = _call(PACKED, _attr(64, BR | _cabi.ATTR_FP8_FOLDED_SCORES), is_causal=1)
    assert rc == -1, (rc, err)
    rc, err = _call(PACKED, _attr(-3, BR), is_causal=1)
    assert rc == -1 and b"SageLaunchAttr.window" in err and b"-3" in err, (rc, err)


@pytest.mark.parametrize("name", [n for n in rej.ATTN if n != PACKED])
@pytest.mark.parametrize("causal", [0, 1])
def test_every_other_entry_point_refuses_a_window_with_the_flag_set(name, causal):
    """The kv_lens entry takes a window of its own and then refuses the flag; every other entry refuses the window first."""
    rc, err = _call(name, _attr(64, BR), **({} if name.endswith("_masked") else dict(is_causal=causal)))
    assert rc == -1 and (b"SageLaunchAttr.window" in err or b"SAGE_ATTR_CAUSAL_BOTTOM_RIGHT" in err), (rc, err)
    if name != rej.KVLENS:
        assert b"SageLaunchAttr.window" in err, (rc, err)


def test_sixteen_entries_refuse_and_one_honours():
    assert PACKED in rej.ATTN and len([n for n in rej.ATTN if n != PACKED]) == 16


# ---------------------------------------------------------------------------------------------- the loop bounds against the predicate
def _check_item(lq, lk, W, qblk, b, stats):
    s = lk - lq
    r0, r1 = 128 * qblk, min(lq, 128 * qblk + 128)                 # the rows of the block that exist
    kc0, n = b["kc0"], b["n_iters"]
    assert kc0 % 64 == 0 and 0 <= kc0 and (kc0 == 0 or kc0 < lk) and b["lk"] == max(lk - kc0, 0) and b["kchunk0"] == kc0 - s
    assert 0 <= n <= (b["lk"] + 63) // 64 and 0 <= b["nh"] <= min(n, 3)
    # the keys the block's rows see: row i sees [max(0, s + i - W + 1), min(lk - 1, s + i)]
    first = max(0, s + r0 - W + 1)                                 # of the block's first row: the smallest of all
    last = min(lk - 1, s + r1 - 1)                                 # of the block's last row: the largest of all
    seeing = [i for i in range(r0, r1) if max(0, s + i - W + 1) <= min(lk - 1, s + i)]      # rows with a key
    if seeing:
        lo = min(max(0, s + i - W + 1) for i in seeing)
        assert first <= lo and kc0 <= lo and last < kc0 + 64 * n, (lq, lk, W, qblk, b)      # every visible key lies in a tile that runs
    else:
        stats["front"] += 1
    # no tile in front of kc0 is requested (tile indices start at 0 = kc0), and kc0 is tight: the first row's first key, if it has one
    # behind key 0, lies in tile 0
    if kc0 > 0:
        assert kc0 <= s + r0 - W + 1 < kc0 + 64, (lq, lk, W, qblk, b)
        stats["shifted"] += 1
    assert n == 0 or kc0 + 64 * (n - 1) <= s + 128 * qblk + 127      # no tile wholly behind the block's diagonal runs
    t = rvw.tiles_run(b)
    assert sorted(t["head"] + t["steady"] + t["diag"] + t["general"]) == list(range(n)), (lq, lk, W, qblk, b, t)
    cut_from = s + (r1 - 1) - W + 1                                # the first key of the last row that exists: tiles holding keys in front of it cut a row
    for tile in t["steady"]:
        k0 = kc0 + 64 * tile
        assert k0 + 64 <= lk, (lq, lk, W, qblk, b)                           # whole
        assert k0 + 63 <= s + r0, (lq, lk, W, qblk, b)                       # behind no row's diagonal: all 128 rows of the block, those past Lq too
        assert k0 >= cut_from, (lq, lk, W, qblk, b)                          # cut by no window of a row that exists
        assert tile + 2 < n                                                  # (the pipelined loop requests two tiles ahead)
    stats["steady"] += len(t["steady"])
    for tile in t["head"]:
        assert kc0 + 64 * tile < cut_from                                    # a head tile does cut a row
    for tile in t["general"] + t["diag"] + t["steady"]:
        assert kc0 + 64 * tile >= cut_from                                   # nothing behind the head tiles does
    if b["diag_ok"]:
        stats["diag"] += 1
        assert (kc0 - s) % 64 == 0 and t["diag"] == [n - 2, n - 1] and kc0 + 64 * n <= lk, (lq, lk, W, qblk, b)
        assert s + r0 - kc0 >= 0, (lq, lk, W, qblk, b)                       # every row of the block sees the item's key 0 side of its diagonal
        assert b["nh"] <= max(b["n_steady"], 0)
        # each row's diagonal key lies in the two tiles or behind them, and its window reaches back to the first of them or further
        assert kc0 + 64 * (n - 2) >= cut_from
    if b["nh"]:
        stats["head"] += 1
    if b["nh"] and t["steady"]:
        stats["head_then_steady"] += 1


def test_loop_bounds_cover_the_predicate():
    """20 000 seeded (Lq, Lk, W, query block): every visible key lies in a tile that runs; no tile in front of kc0 is requested and kc0 is
    tight; steady tiles are whole, behind no diagonal of the block's 128 rows, and cut by no window of a row that exists (the kernel forms
    the head tiles from the block's last EXISTING row, as the dense window kernel does: a decode row would otherwise pay two more head
    tiles; rows past Lq are never stored); whenever diag_ok holds, its precondition holds."""
    rng = np.random.default_rng(313)
    stats = dict(front=0, shifted=0, steady=0, diag=0, head=0, head_then_steady=0)
    for t in range(20000):
        kind = t % 5
        lq, lk = int(rng.integers(1, 1200)), int(rng.integers(0, 2400))
        W = int(rng.choice([1, 2, 63, 64, 65, 100, 128, 192, 256, 448, 1000, 4096, 2 ** 30])) if t % 3 else int(rng.integers(1, 1500))
        if kind == 1:
            lk = max(0, lq + 64 * int(rng.integers(-6, 30)))        # offsets that are multiples of 64
        elif kind == 2:
            lq, lk = int(rng.integers(1, 40)), int(rng.integers(0, 3000))      # decode / verification rows
        elif kind == 3:
            lk = int(rng.integers(0, lq + 1))                       # more rows than keys
        elif kind == 4:
            lk = lq                                                  # Lq = Lk
        qblk = int(rng.integers(0, (lq + 127) // 128))
        _check_item(lq, lk, W, qblk, rvw.loop_bounds(lq, lk, W, qblk), stats)
    print(stats)
    assert min(stats.values()) > 300, stats


def test_a_window_that_cuts_no_row_has_the_unwindowed_bounds():
    rng = np.random.default_rng(314)
    for _ in range(3000):
        lq, lk = int(rng.integers(1, 1500)), int(rng.integers(0, 3000))
        for qblk in range((lq + 127) // 128):
            for W in (lq + lk, 2 ** 30 - 1, 2 ** 30):
                b, u = rvw.loop_bounds(lq, lk, W, qblk), rb.loop_bounds(lq, lk, qblk)
                assert b["kc0"] == 0 and b["nh"] == 0 and all(b[x] == u[x] for x in ("kchunk0", "n_iters", "n_steady", "nd", "diag_ok")), (lq, lk, W)


def test_loop_bounds_of_the_tested_batch():
    """The shapes of tests/test_gpu_varlen_window.py's batch reach what its table says."""
    B = lambda lq, lk, W, j: rvw.loop_bounds(lq, lk, W, j)
    T = lambda lq, lk, W, j: {k: len(v) for k, v in rvw.tiles_run(B(lq, lk, W, j)).items()}
    # (448, 448): interior blocks start behind key 0, run head tiles and the diagonal
    assert [B(448, 448, 100, j)["kc0"] for j in range(4)] == [0, 0, 128, 256] and [B(448, 448, 1, j)["kc0"] for j in range(4)] == [0, 128, 256, 384]
    assert T(448, 448, 100, 2) == dict(head=3, steady=0, diag=0, general=1) and T(448, 448, 192, 2) == dict(head=2, steady=1, diag=2, general=0)
    assert T(448, 448, 448, 3) == dict(head=0, steady=5, diag=2, general=0) and B(448, 448, 192, 2)["kc0"] == 64
    # (128, 568), offset 440: three general tiles on the diagonal
    assert T(128, 568, 448, 0) == dict(head=2, steady=4, diag=0, general=3) and B(128, 568, 100, 0)["kc0"] == 320
    assert T(128, 568, 192, 0) == dict(head=3, steady=0, diag=0, general=3)
    # (128, 1024), offset 896: head + steady + pipelined diagonal tiles behind kc0 > 0
    b = B(128, 1024, 448, 0)
    assert b["kc0"] == 448 and b["diag_ok"] and T(128, 1024, 448, 0) == dict(head=2, steady=5, diag=2, general=0)
    assert B(128, 1024, 192, 0)["kc0"] == 704 and T(128, 1024, 192, 0) == dict(head=2, steady=1, diag=2, general=0)
    # decode, decode with W > Lk, verification
    assert B(1, 1000, 100, 0)["kc0"] == 896 and T(1, 1000, 100, 0) == dict(head=1, steady=0, diag=0, general=1)
    assert T(1, 1000, 448, 0) == dict(head=1, steady=4, diag=0, general=3) and B(1, 1000, 1, 0)["kc0"] == 960
    assert B(1, 50, 100, 0)["kc0"] == 0 and T(1, 50, 100, 0) == dict(head=0, steady=0, diag=0, general=1)
    assert B(5, 700, 192, 0)["kc0"] == 448 and T(5, 700, 192, 0) == dict(head=1, steady=0, diag=0, general=3)
    # rows in front of key 0 sharing a block with rows that see keys; a lone key; no keys
    assert [B(300, 130, 100, j)["n_iters"] for j in range(3)] == [0, 2, 3] and rvw.rows_without_keys(300, 130, 100) == 170
    assert T(300, 130, 1, 1) == dict(head=2, steady=0, diag=0, general=0) and B(300, 130, 1, 2)["kc0"] == 64
    assert B(7, 1, 1, 0)["n_iters"] == 1 and rvw.rows_without_keys(7, 1, 1) == 6 and B(64, 0, 100, 0)["n_iters"] == 0
    assert T(128, 128, 448, 0) == dict(head=0, steady=0, diag=2, general=0) and T(128, 128, 1, 0) == dict(head=2, steady=0, diag=0, general=0)
    for W in WINDOWS:
        assert any(B(lq, lk, W, j)["kc0"] > 0 for lq, lk in BATCH for j in range((lq + 127) // 128))
        assert any(B(lq, lk, W, j)["nh"] > 0 for lq, lk in BATCH for j in range((lq + 127) // 128))


# ---------------------------------------------------------------------------------------------- the build
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_packed_window_units_build_within_the_family_targets():
    """The units are in the Makefile's SRCS; each holds the causal two-level exact-score kernel for fp16 and bf16 q (QF 3 / 4), with and
    without the ticket loop (CPERS): four kernels per unit, no scratch and no spilled VGPR.  D = 128: two waves per SIMD.  D = 64: three for
    the plain kernels; the ticket kernels need 172 VGPRs, four more than three waves leave, and are built for two rather than
    with scratch."""
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
            # D, FP8 PV, causal, per-block k scales, two-level, no mask, the exact form ... WINDOW, QSTART, no KVLEN; QF 3 / 4 and CPERS or not
            f = forms[name]
            assert f == tbr.kf.form(128 if d128 else 64, pv_fp8=True, causal=True, two_level=True, window=True, qstart=True, qf=f["qf"], cpers=f["cpers"]), name
            assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0, (name, res)
            tickets = f["cpers"]
            want = 2 if d128 or tickets else 3
            assert res["Occupancy"] >= want and res["VGPRs"] <= (256 if want == 2 else 168), (name, res)
        assert {(f["qf"] == 3, f["cpers"]) for f in forms.values()} == {(a, b) for a in (True, False) for b in (True, False)}, sorted(mine)
        assert all((f["qf"] == 3) != (f["qf"] == 4) for f in forms.values()), sorted(mine)


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_packed_window_units_pass_the_mfma_hazard_lint():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_hazard_lint as lint
    assert lint.UNITS_PACKED_WINDOW == UNITS
    assert not set(UNITS) & set(lint.UNITS + lint.UNITS_PAIR + lint.UNITS_WINDOW + lint.UNITS_PACKED_BR)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as ex:
        results = dict(zip(UNITS, ex.map(lambda u: lint.lint(lint.listing(u)), UNITS)))
    for unit, (findings, n_mfma) in results.items():
        assert n_mfma >= 200, (unit, n_mfma)                   # (four kernels: the walk did see the pipelined loops)
        assert not findings, (unit, findings[:5])
