"""CPU: the listed step call on the paged KV cache -- C boundary, Python interface, the list arithmetic, the dealing rules, the build
(include/sage_kvlist_gfx950.h, sageattention_amd/_cabi_kvlist.py, sageattention_amd/paged_kv_list.py, csrc/sage_step_list.h,
csrc/sage_attn_d{128,64}_{f8pl,f8plg}.hip).  The new header's prototypes are the new binding's table, the library exports them, every argument
error of the entry returns -1 with its message before anything touches a GPU and in the header's order, the Python layer raises ValueError
before any work, the list arithmetic holds over hostile words (a stand-alone program under AddressSanitizer and UBSan), the host plan gives the
hand-checked lists, the two dealing rules hand every item to exactly one workgroup, each new unit holds exactly the list kernels of the forms
it is instantiated from, without scratch and at its form's occupancy -- and none of it moved what the other headers, bindings and units pin."""
import ctypes
import itertools
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import util  # noqa: F401  (sys.path)
import sageattention_amd as sa
import test_build_resources as tbr
import test_kv_step_host as step
import test_kv_varlen_host as varlen
import test_paged_kv_host as paged
from sageattention_amd import _cabi, _cabi_kvcache, _cabi_kvfork, _cabi_kvlist, _cabi_kvpaged, _cabi_kvpsplit, _cabi_kvpvarlen, _cabi_kvstep
from sageattention_amd.kv_cache import QuantizedKVCache
from sageattention_amd.paged_kv_list import sageattn_kvcache_step_listed
from test_kv_cache_host import MAIN_HEADER, _prototypes, _text
from test_paged_kv_host import listed  # noqa: F401  (the fixture: the forms of the lists the paged units are instantiated from)

kf = tbr.kf
ROOT = tbr.ROOT
CSRC = os.path.join(ROOT, "sageattention_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "sage_kvlist_gfx950.h")
ENTRIES = ["sage_kvlist_abi_version", "sage_kvlist_attn", "sage_kvlist_plan", "sage_kvlist_plan_host", "sage_kvlist_ws_bytes"]
_Dev = varlen._Dev
HDR = 16


def test_binding_is_the_header():
    protos = _prototypes(HEADER, "SAGE_KVLIST_API")
    assert sorted(protos) == sorted(_cabi_kvlist.SYMBOLS) == ENTRIES
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_kvlist.SYMBOLS[name]
        assert res is paged._ctype(ret), f"{name}: returns {ret}, bound as {res}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters declared, {len(argtypes)} bound"
        for i, (ctype, bound) in enumerate(zip(params, argtypes)):
            assert bound is paged._ctype(ctype), f"{name}: parameter {i} ({ctype}) bound as {bound}"
    version = int(re.search(r"#define\s+SAGE_KVLIST_ABI_VERSION\s+(\d+)", _text(HEADER)).group(1))
    assert version == 1 == _cabi_kvlist.ABI_VERSION
    rest = re.sub(r"SAGE_KVLIST_API", "", _text(HEADER))
    assert "SAGE_API" not in rest and "SAGE_KVSTEP_API" not in rest and "SAGE_KVPVARLEN_API" not in rest          # an export macro of its own
    assert "sage_kvlist_gfx950.h" in open(os.path.join(CSRC, "Makefile")).read()
    # the entry takes sage_kvstep_attn's arguments, argument for argument, followed by the workspace
    theirs = _prototypes(step.HEADER, "SAGE_KVSTEP_API")["sage_kvstep_attn"]
    assert protos["sage_kvlist_attn"] == (theirs[0], theirs[1] + ["int32_t *", "int64_t"])
    assert _cabi_kvlist.SYMBOLS["sage_kvlist_attn"][1][:-2] == _cabi_kvstep.SYMBOLS["sage_kvstep_attn"][1]
    # the two plan entries differ in their last arguments alone
    assert protos["sage_kvlist_plan"][1][:-1] == protos["sage_kvlist_plan_host"][1][:-2]


def test_library_exports_the_entries_and_the_other_boundaries_did_not_move():
    lib = ctypes.CDLL(_cabi.LIB_PATH)
    for name in _cabi_kvlist.SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
    assert _cabi_kvlist.load() is _cabi.load()                       # one library, bound behind _cabi.load()
    assert _cabi_kvlist.load().sage_kvlist_abi_version() == 1
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22
    assert len(_prototypes(MAIN_HEADER, "SAGE_API")) == 56 and len(_cabi.SYMBOLS) == 56
    assert sorted(_cabi_kvstep.SYMBOLS) == step.ENTRIES and _cabi_kvstep.load().sage_kvstep_abi_version() == 1
    assert sorted(_prototypes(step.HEADER, "SAGE_KVSTEP_API")) == step.ENTRIES
    assert sorted(_cabi_kvpvarlen.SYMBOLS) == varlen.ENTRIES and len(varlen.ENTRIES) == 3 and _cabi_kvpvarlen.load().sage_kvpvarlen_abi_version() == 1
    assert sorted(_cabi_kvpaged.SYMBOLS) == paged.ENTRIES and _cabi_kvpaged.load().sage_kvpaged_abi_version() == 1
    assert _cabi_kvcache.load().sage_kvcache_abi_version() == 1 and _cabi_kvfork.load().sage_kvfork_abi_version() == _cabi_kvfork.ABI_VERSION
    assert _cabi_kvpsplit.load().sage_kvpsplit_abi_version() == _cabi_kvpsplit.ABI_VERSION
    # no symbol starts with another binding's prefix, either way
    others = [n for b in (_cabi, _cabi_kvcache, _cabi_kvpaged, _cabi_kvfork, _cabi_kvpsplit, _cabi_kvpvarlen, _cabi_kvstep) for n in b.SYMBOLS]
    assert not any(n.startswith("sage_kvlist") for n in others)
    for prefix in ("sage_kvstep", "sage_kvpvarlen", "sage_kvpaged", "sage_kvpsplit", "sage_kvfork", "sage_kvcache"):
        assert not any(n.startswith(prefix) for n in _cabi_kvlist.SYMBOLS)
    assert not hasattr(sa, "sageattn_kvcache_step_listed") and "sageattn_kvcache_step_listed" not in sa.__all__
    assert not hasattr(sa, "paged_kv_list") or "paged_kv_list" not in sa.__all__


# ---- argument errors of the entry, in the header's order ------------------------------------------------------------------------------------
_DEFAULT = object()


def _attn(lib, p, attr=_DEFAULT, list_ws=_DEFAULT, list_ws_bytes=1 << 20, **kw):
    a = dict(q=p, k_int8=p, v_image=p, o=p, lse=None, k_scale=p, v_scale=p, kv_lens=p, cu_seqlens_q=p, block_table=p, bt_stride=2, num_pages=4,
             page_size=64, max_pages_per_seq=2, B=1, Hq=2, Hkv=1, total_q=1, max_seqlen_q=1, D=64, q_sl=128, q_sh=64, k_sb=4096, k_sh=4096, k_sl=64,
             o_sl=128, o_sh=64, lse_sh=1, is_causal=1, sm_scale_log2=1.0, q_dtype=0, out_dtype=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    if attr is _DEFAULT:
        attr = _cabi.launch_attr(q_start=_Dev(p))
    if list_ws is _DEFAULT:
        list_ws = p
    return lib.sage_kvlist_attn(*a.values(), _cabi.attr_arg(attr), list_ws, list_ws_bytes), lib.sage_last_error()


def _attn_order(p):
    """sage_kvstep_attn's checks in its order, under this entry's name; then the workspace and the plan's batch limit."""
    e = b"sage_kvlist_attn: "
    theirs = [(kw, match.replace(b"sage_kvstep_attn: ", e)) for kw, match in step._attn_order(p)]
    assert sum(match.startswith(e) for _, match in theirs) == 10
    return theirs + [(dict(list_ws=None), e + b"list_ws must be int32 device memory, 4-byte aligned"),
                     (dict(list_ws_bytes=4 * HDR), e + b"list_ws holds 64 bytes, sage_kvlist_ws_bytes(B, total_q, max_seqlen_q) = "),
                     (dict(B=1025), e + b"B must be at most 1024")]


def test_every_argument_error_returns_minus_one_in_the_headers_order():
    lib = _cabi_kvlist.load()
    buf, p = paged._aligned_buffer()
    checks = _attn_order(p)
    for kw, match in checks:                                         # each violation alone gives its own message, under the entry's own name
        rc, msg = _attn(lib, p, **kw)
        assert rc == -1 and match in msg and b"sage_kvstep" not in msg and b"sage_kvpvarlen" not in msg.replace(b"sage_kvpvarlen_attn takes such a call", b""), (kw, rc, msg)
    rc, msg = _attn(lib, p, list_ws=p + 2)
    assert rc == -1 and b"sage_kvlist_attn: list_ws must be int32 device memory, 4-byte aligned" in msg
    covered = set()
    for (i, (kw_i, match_i)), (j, (kw_j, _)) in itertools.combinations(enumerate(checks), 2):
        if set(kw_i) & set(kw_j):                                    # two values for one argument do not fit into one call
            continue
        rc, msg = _attn(lib, p, **kw_i, **kw_j)
        assert rc == -1 and match_i in msg, (kw_i, kw_j, rc, msg)
        covered.add((i, j))
    # (B = 0 and B = 1025 are two values of one argument: the pair (B and Hkv, table alignment) .. is covered as in the step call's test, and the
    #  workspace checks stand behind every one of its checks)
    assert all((i, i + 1) in covered for i in range(len(checks) - 1)), sorted(covered)
    with pytest.raises(ValueError):
        _cabi.check(-1, "sage_kvlist_attn")
    # the attributes the step call refuses by name, under this entry's
    ws, qs = _Dev(p), _Dev(p)
    e = b"sage_kvlist_attn: "
    for attr, match in ((_cabi.launch_attr(ws, kv_split=2, q_start=qs), e + b"SAGE_ATTR_KV_SPLIT is not supported on a paged cache"),
                        (_cabi.launch_attr(folded_scores=True, q_start=qs), e + b"SAGE_ATTR_FP8_FOLDED_SCORES is not supported on a paged cache"),
                        (_cabi.launch_attr(ws, force_persistent=True, q_start=qs), e + b"SAGE_ATTR_FORCE_PERSISTENT is not supported on a paged cache"),
                        (_cabi.launch_attr(gqa_pack=True, q_start=qs), e + b"SAGE_ATTR_GQA_PACK is not taken (the entry packs the decode rows of a GQA group on its own)"),
                        (_cabi.launch_attr(window=5), e + b"SageLaunchAttr.q_start is required"),
                        (None, e + b"SageLaunchAttr.q_start is required")):
        rc, msg = _attn(lib, p, attr=attr)
        assert rc == -1 and match in msg, (rc, msg)
    # ... and the step call kept its own name
    rc, msg = step._attn(_cabi_kvstep.load(), p, attr=None)
    assert rc == -1 and b"sage_kvstep_attn: SageLaunchAttr.q_start is required" in msg
    del buf


def test_the_plan_entries_check_their_arguments_and_size_the_workspace():
    lib = _cabi_kvlist.load()
    # 4 * (16 + B + 2 * bound), bound = min(B * ceil(max / 128), total // 128 + min(B, total // 33)), 0 when no sequence can be a chunk
    for (B, total, max_q), bound in (((4, 171, 130), 5), ((4, 171, 32), 0), ((4, 32, 130), 0), ((1, 1, 1), 0), ((11, 501, 260), 14), ((2, 4096, 4096), 34),
                                     ((128, 2172, 512), 81), ((3, 1000, 128), 3)):
        assert lib.sage_kvlist_ws_bytes(B, total, max_q) == 4 * (HDR + B + 2 * bound), (B, total, max_q)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert lib.sage_kvlist_ws_bytes(*bad) == -1 and b"sage_kvlist_ws_bytes" in lib.sage_last_error()
    buf, p = paged._aligned_buffer()
    ok = dict(cu=p, kv=p, qs=p, B=1, total_q=1, max_seqlen_q=1, capacity=64, window=0, Hq=2, Hkv=1, D=64, ws=p, nbytes=4096)
    for kw, match in ((dict(cu=None), b"null cu_seqlens_q, kv_lens or q_start"), (dict(qs=p + 2), b"4-byte aligned"), (dict(B=0), b"B must be in 1 .. 1024"),
                      (dict(B=1025), b"B must be in 1 .. 1024"), (dict(capacity=0), b"at least 1"), (dict(window=-1), b"window = -1"),
                      (dict(Hq=3, Hkv=2), b"divisible"), (dict(D=96), b"head_dim must be 64 or 128"), (dict(ws=None), b"list_ws is 68 bytes"),
                      (dict(nbytes=64), b"list_ws is 68 bytes")):
        a = dict(ok, **kw)
        for entry, extra in (("sage_kvlist_plan", (None,)), ("sage_kvlist_plan_host", (None, None))):
            rc = getattr(lib, entry)(*a.values(), *extra)
            err = lib.sage_last_error()
            assert rc == -1 and match in err, (entry, kw, err)
            assert match.startswith(b"head_dim") or err.startswith(entry.encode() + b": "), (entry, kw, err)
    del buf


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------------
def test_value_errors_before_any_work():
    c = paged._cache(seeded=True)                # B 2, Hkv 2, D 64, fp16, pages of 128, on the CPU
    q = torch.zeros(5, 4, 64, dtype=torch.float16)
    cu = torch.tensor([0, 2, 5], dtype=torch.int32)
    contiguous = QuantizedKVCache.allocate(2, 2, 64, 64, torch.float16, "cpu")
    for args, kw, match in (
            ((q, contiguous, cu, 3), {}, "sageattn_kvcache_step_listed takes a PagedQuantizedKVCache"),
            ((q, "cache", cu, 3), {}, "sageattn_kvcache_step_listed takes a PagedQuantizedKVCache"),
            ((q, paged._cache(seeded=False), cu, 3), {}, "no statistics"),
            ((q[:, :2], c, cu, 3), {}, r"sageattn_kvcache_step_listed packs the query heads of a GQA group: Hq / Hkv must be at least 2 \(got 2 / 2\)"),
            ((torch.zeros(5, 3, 64, dtype=torch.float16), c, cu, 3), {}, "divisible"),
            ((q.unsqueeze(0), c, cu, 3), {}, "3-D"),
            ((q.float(), c, cu, 3), {}, "dtype"),
            ((q.to("meta"), c, cu, 3), {}, "device"),
            ((torch.zeros(5, 4, 128, dtype=torch.float16), c, cu, 3), {}, "must be"),
            ((torch.zeros(0, 4, 64, dtype=torch.float16), c, cu, 3), {}, "must be"),
            ((q, c, cu.long(), 3), {}, "cu_seqlens_q must be an int32 tensor"),
            ((q, c, cu[:2], 3), {}, r"shape \[B \+ 1\]"),
            ((q, c, cu.to("meta"), 3), {}, "device"),
            ((q, c, cu, 0), {}, "max_seqlen_q must be a positive int"),
            ((q, c, cu, True), {}, "max_seqlen_q must be a positive int"),
            ((q, c, cu, 3), dict(window_size=(70,)), "window_size"),
            ((q, c, cu, 3), dict(window_size=(70, 5)), "window_size"),
            ((q, c, cu, 3), dict(q_start=torch.zeros(3, dtype=torch.int32)), r"shape \[B\]"),
            ((q, c, cu, 3), dict(q_start=torch.zeros(2)), "q_start must be an int"),
            ((q, c, cu, 3), dict(return_plan=True, window_size=(70, 5)), "window_size")):
        with pytest.raises(ValueError, match=match):
            sageattn_kvcache_step_listed(*args, **kw)
    for kw in (dict(pack_gqa=True), dict(num_splits=2)):
        with pytest.raises(TypeError):
            sageattn_kvcache_step_listed(q, c, cu, 3, **kw)
    # the modules it stands beside are what they were: it imports their helpers, they know nothing of it
    for name in ("paged_kv_step.py", "paged_kv_varlen.py"):
        assert "kv_list" not in open(os.path.join(ROOT, "sageattention_amd", name)).read() and "listed" not in open(os.path.join(ROOT, "sageattention_amd", name)).read()


# ---- the list arithmetic ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_lists_hold_over_hostile_words_under_the_sanitizers(tmp_path):
    """tests/step_list_main.cpp: a program of its own (no GPU, nothing loaded into this process), AddressSanitizer and UBSan on the host."""
    exe = tmp_path / "step_list"
    # (host code only: the file is compiled as C++, every sanitizer option goes to the host compilation by name)
    host = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    out = subprocess.run([tbr.HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", *host, "-I", CSRC,
                          os.path.join(ROOT, "tests", "step_list_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    syms = subprocess.run(["nm", str(exe)], capture_output=True, text=True, timeout=60).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the program was built without the sanitizers"
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    assert run.returncode == 0 and "every rank once, weights in order, all inside" in run.stdout and "runtime error" not in run.stderr and \
        "AddressSanitizer" not in run.stderr, (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    # one definition: the header includes nothing beyond the clamp and the work order, states no clamp of its own, and the kernel, the launcher
    # and the C boundary read it
    text = open(os.path.join(CSRC, "sage_step_list.h")).read()
    assert re.findall(r"#include\s+(\S+)", text) == ['"sage_ragged.h"', '"sage_work_order.h"']
    assert text.count("ragged_band(") == 2 and "q1 - q0" not in text
    for user in ("sage_kv_list_plan.hip", "sage_attn.hip", "sage_cabi.hip"):
        assert '#include "sage_step_list.h"' in open(os.path.join(CSRC, user)).read(), user
    # the body and the kernel header are what tests/test_kv_step_host.py pins; the fifth entry stands in a header of its own
    body = open(os.path.join(CSRC, "sage_attn_body.h")).read()
    assert body.count("ragged_rows(") == 2 and body.count("ragged_band(") == 1 and body.count("if constexpr (LIST") == 2
    kernel_h = open(os.path.join(CSRC, "sage_attn_kernel.h")).read()
    assert "SAGE_ATTN_BODY_LIST" not in kernel_h and kernel_h.count("#define SAGE_ATTN_BODY_BAND false") == 3
    list_h = open(os.path.join(CSRC, "sage_attn_list_kernel.h")).read()
    assert list_h.count("#define SAGE_ATTN_BODY_LIST true") == 1 and list_h.count("#define SAGE_ATTN_BODY_BAND true") == 1


def _plan(counts, ctx, cap, max_q, Hq=8, Hkv=2, D=128, window=0, q_start=None):
    lib = _cabi_kvlist.load()
    B, total = len(counts), sum(counts)
    cu = np.array([sum(counts[:b]) for b in range(B + 1)], dtype=np.int32)
    kv = np.array(ctx, dtype=np.int32)
    qs = np.array(q_start, dtype=np.int32) if q_start is not None else (np.clip(kv, 0, cap) - np.array(counts)).astype(np.int32)      # bottom-right
    nbytes = lib.sage_kvlist_ws_bytes(B, total, max_q)
    ws = np.full(nbytes // 4, -1, dtype=np.int32)
    dg, cg = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.sage_kvlist_plan_host(cu.ctypes.data, kv.ctypes.data, qs.ctypes.data, B, total, max_q, cap, window, Hq, Hkv, D, ws.ctypes.data, nbytes,
                                   ctypes.byref(dg), ctypes.byref(cg))
    assert rc == 0, lib.sage_last_error()
    nd, nc = int(ws[0]), int(ws[1])
    return dict(hdr=ws[:HDR].tolist(), decode=ws[HDR:HDR + nd].tolist(), chunk=ws[HDR + B:HDR + B + 2 * nc].reshape(nc, 2).tolist(),
                rest=ws[HDR + nd:HDR + B].tolist() + ws[HDR + B + 2 * nc:].tolist(), grids=(dg.value, cg.value))


def test_the_host_plan_on_hand_checked_steps():
    # counts (1, 40, 0, 130) over contexts (640, 64, 128, 601), bottom-right: sequence 0 decodes (ten tiles), sequence 2 is idle.  Chunk weights,
    # min(2 j + 2 + ceil((keys - rows) / 64), ceil(keys / 64)): sequence 3 (601 keys, 130 rows): min(2 + 8, 10) = 10 and min(4 + 8, 10) = 10;
    # sequence 1 (64 keys, 40 rows): min(2 + 1, 1) = 1.  Equal weights: the later block first.
    r = _plan((1, 40, 0, 130), (640, 64, 128, 601), 1024, 130)
    assert r["decode"] == [0] and r["chunk"] == [[3, 1], [3, 0], [1, 0]]
    assert r["hdr"][:2] == [1, 3] and r["hdr"][4] == 0 and r["hdr"][5] == 3 and r["hdr"][6] == 601 and r["hdr"][7:] == [0] * 9
    assert set(r["rest"]) == {-1}                                     # entries past the two counts are not written
    assert r["grids"] == (8, 8 * 5)                                   # one octet of (sequence, kv head) units; 5 = min(4 * 2, 171 // 128 + min(4, 171 // 33)) slots of Hq = 8 heads
    # a window of 71 keys caps a chunk item at ceil((71 + 128) / 64) + 1 = 5 tiles: sequence 3's blocks both weigh 5, still ahead of sequence 1; the
    # decode weight of sequence 0 is capped alike, which changes nothing with one decode sequence
    w = _plan((1, 40, 0, 130), (640, 64, 128, 601), 1024, 130, window=71)
    assert w["decode"] == [0] and w["chunk"] == [[3, 1], [3, 0], [1, 0]]
    # ... and under the cap a long context no longer outranks a shorter one that reaches it: (600 keys, 40 rows) weighs min(2 + 9, 10) = 10 alone,
    # 5 under the window -- as (320 keys, 40 rows) does with min(2 + 5, 5) = 5: the earlier sequence first
    assert _plan((40, 40), (320, 600), 1024, 40)["chunk"] == [[1, 0], [0, 0]]
    assert _plan((40, 40), (320, 600), 1024, 40, window=71)["chunk"] == [[0, 0], [1, 0]]
    # decode sequences by ceil(keys / 64) descending, ties by index; 32 rows decode, 33 do not; a sequence cut to max_seqlen_q = 32 rows decodes
    d = _plan((1, 32, 33, 1, 2, 40), (65, 640, 200, 64, 0, 100), 1024, 32)
    assert d["decode"] == [1, 2, 0, 5, 3, 4] and d["chunk"] == [] and d["grids"] == (8 * 2, 0)        # weights 10, 4, 2, 2, 1, 0 (sequence 2: 200 keys, cut to 32 rows)
    d = _plan((1, 32, 33, 1, 2, 40), (65, 640, 200, 64, 0, 100), 1024, 40)
    assert d["decode"] == [1, 0, 3, 4] and d["chunk"] == [[2, 0], [5, 0]]                             # chunk weights min(2 + 3, 4) = 4 and min(2 + 1, 2) = 2
    # an explicit q_start moves the diagonal: rows in front of key 0 weigh nothing, rows past the last key the whole context
    s = _plan((40, 40, 1), (640, 640, 640), 1024, 40, q_start=(-40, 5000, -1))
    assert s["chunk"] == [[1, 0], [0, 0]] and s["decode"] == [2]
    # a malformed prefix array: four overlapping sequences of 170 rows in 171 give eight blocks, the bound is five -- the five heaviest stay
    lib = _cabi_kvlist.load()
    cu = np.array([0, 170, 0, 170, 0], dtype=np.int32)
    cu2 = np.array([0, 170, 340, 510, 680], dtype=np.int32)           # (beyond total_q: clamped to one sequence of 130 rows and nothing behind it)
    kv, qs = np.array([640] * 4, dtype=np.int32), np.array([500] * 4, dtype=np.int32)
    for words, n_all in ((cu, 4), (cu2, 2)):
        nbytes = lib.sage_kvlist_ws_bytes(4, 171, 130)
        ws = np.full(nbytes // 4, -1, dtype=np.int32)
        assert lib.sage_kvlist_plan_host(words.ctypes.data, kv.ctypes.data, qs.ctypes.data, 4, 171, 130, 1024, 0, 8, 2, 128, ws.ctypes.data, nbytes, None, None) == 0
        assert ws[5] == n_all and ws[1] == min(n_all, 5) and ws.shape == (HDR + 4 + 10,)


# ---- the dealing rules ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,B", [(8, 2, 4), (12, 2, 4), (4, 2, 4), (8, 2, 11)])
def test_every_item_of_both_grids_is_taken_exactly_once(Hq, Hkv, B):
    lib = _cabi.load()
    group = Hq // Hkv
    ngb = (group + 3) // 4
    # decode: units (list rank, kv head) round-robin over the XCDs, the blocks of a unit on one XCD -- the kernel's statements, restated
    grid = 8 * ((B * Hkv + 7) // 8) * ngb
    for n_decode in range(B + 1):
        seen = {}
        for bid in range(grid):
            xcd, idx = bid & 7, bid >> 3
            unit, gb = (idx // ngb) * 8 + xcd, idx % ngb
            if unit >= n_decode * Hkv:
                continue
            item = (unit // Hkv, unit % Hkv, gb)
            assert item not in seen and bid & 7 == seen.get(("xcd",) + item[:2], bid & 7)
            seen[item] = bid
            seen[("xcd",) + item[:2]] = bid & 7                       # (the blocks of a unit share its XCD)
        assert {k for k in seen if k[0] != "xcd"} == {(r, hk, gb) for r in range(n_decode) for hk in range(Hkv) for gb in range(ngb)}
    # chunks: a dense launch over Hq heads of nitems items, dealt by work_item() with nwg from the header; the host grid is sized by the bound
    counts = ([1, 40, 0, 130] if B == 4 else [1, 130, 1, 0, 33, 1, 2, 40, 1, 32, 260])
    for D in (128, 64):
        for n_keep in range(len(counts) + 1):                        # fewer and fewer chunk sequences, down to none
            c = [n if n <= 32 or sum(1 for m in counts[:i + 1] if m > 32) <= n_keep else 1 for i, n in enumerate(counts)]
            r = _plan(c, [300] * B, 320, max(c), Hq, Hkv, D)
            nitems, grp, fold, left = r["hdr"][1:5]
            assert left == Hq % 8 and fold in (0, 1) and 1 <= grp
            nwg = 8 * (left * ((nitems + 7) // 8) + (Hq >> 3) * nitems)
            assert nwg <= r["grids"][1] or max(c) <= 32
            seen = set()
            head, qrank = ctypes.c_int(-1), ctypes.c_int(-1)
            for bid in range(nwg):
                took = lib.sage_debug_work_item(bid, nwg, Hq, nitems, grp, fold, left, ctypes.byref(head), ctypes.byref(qrank))
                assert took in (0, 1), lib.sage_last_error()
                if took:
                    assert 0 <= head.value < Hq and 0 <= qrank.value < nitems and (head.value, qrank.value) not in seen
                    seen.add((head.value, qrank.value))
            assert len(seen) == Hq * nitems and nitems == len(r["chunk"])


# ---- the build ------------------------------------------------------------------------------------------------------------------------------
LIST_UNITS = {"f8pl": ("UNIT_F8Q", "UNIT_F8W"), "f8plg": ("UNIT_F8G",)}
LIST_NAME = r"_ZN4sage27sage_attn_paged_list_kernelILj(\d+)EEEvNS_10AttnParamsENS_9PagedArgsENS_10RaggedArgsENS_8BandArgsE"


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_list_units_hold_the_list_kernels_of_their_lists_without_scratch_or_hazard(listed):  # noqa: F811
    import mfma_hazard_lint as lint
    srcs = [f"sage_attn_d{D}_{u}.hip" for u in LIST_UNITS for D in (128, 64)]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    in_srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert all(s in in_srcs for s in srcs) and "sage_kv_list_plan.hip" in in_srcs
    # the lint's new tuple names them and is disjoint from the others, whose contents stand
    assert lint.UNITS_PAGED_LIST == tuple(srcs)
    rest = (lint.UNITS + lint.UNITS_PAIR + lint.UNITS_WINDOW + lint.UNITS_PACKED_BR + lint.UNITS_PACKED_WINDOW + lint.UNITS_GQA_PACK + lint.UNITS_KV_SPLIT +
            lint.UNITS_PAGED + lint.UNITS_PAGED_SPLIT + lint.UNITS_PAGED_RAGGED + lint.UNITS_PAGED_STEP)
    assert not set(srcs) & set(rest) and len(rest) == 36
    assert lint.UNITS_PAGED_STEP == ("sage_attn_d128_f8pb.hip", "sage_attn_d64_f8pb.hip", "sage_attn_d128_f8pbg.hip", "sage_attn_d64_f8pbg.hip")
    with ThreadPoolExecutor(max_workers=2 * len(srcs)) as ex:
        reports = ex.map(tbr._resource_report, srcs + ["sage_kv_list_plan.hip"])
        lints = ex.map(lambda u: lint.lint(lint.listing(u)), srcs)
        reports, lints = dict(zip(srcs + ["sage_kv_list_plan.hip"], reports)), dict(zip(srcs, lints))
    for u, units in LIST_UNITS.items():
        for D in (128, 64):
            src = f"sage_attn_d{D}_{u}.hip"
            rep = reports[src]
            every = {}
            for unit in units:
                every.update(listed[(unit, D)])
            want = {w: waves for w, waves in every.items() if kf.unpack(w)["qstart"]}
            assert len(want) == 4 and len(every) == (4 if u == "f8pl" else 8)
            assert not [k for k in rep if "sage_attn_kernel" in k or "sage_attn_paged_kernel" in k or "sage_attn_paged_varlen_kernel" in k or
                        "sage_attn_paged_step_kernel" in k], "a kernel of another entry in a list unit"
            assert len(rep) == 4, sorted(rep)
            for name, res in rep.items():
                m = re.fullmatch(LIST_NAME, name)
                assert m, name
                word = int(m.group(1))
                f = kf.unpack(word)
                assert word in want and f["D"] == D and f["causal"] and f["qstart"] and f["kvlen"] and f["pv_fp8"] and not f["seed"], (name, f)
                assert bool(f["gpack"]) == (u == "f8plg") and f["qf"] in (1, 2), (name, f)
                assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0 and res.get("SGPRs Spill", 0) == 0, (name, res)
                assert res["Occupancy"] >= want[word] == (3 if D == 64 else 2), (name, res)          # the form's own bound: no two-wave fallback
            assert {int(re.fullmatch(LIST_NAME, k).group(1)) for k in rep} == set(want)
            assert {kf.unpack(w)["window"] for w in want} == {0, 1} and {kf.unpack(w)["qf"] for w in want} == {1, 2}
            findings, n_mfma = lints[src]
            assert n_mfma >= 100 and not findings, (src, n_mfma, findings[:5])
    plan = reports["sage_kv_list_plan.hip"]
    assert list(plan) == ["_ZN4sage19kv_list_plan_kernelENS_16KvListPlanParamsE"]
    assert all(res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0 for res in plan.values())
    # the step units hold what they held, and the form table is untouched: no form bit, no member of the unit list
    for D in (128, 64):
        for u in ("f8pb", "f8pbg"):
            text = open(os.path.join(CSRC, f"sage_attn_d{D}_{u}.hip")).read()
            assert "launch_attn_step_units" in text and "list_kernel" not in text and "launch_attn_list" not in text
    form_h = open(os.path.join(CSRC, "sage_attn_form.h")).read()
    assert "X(F8) X(F8F) X(F16) X(F8V) X(F8VB) X(F8VBW) X(F8S) X(F8K) X(F8Q) X(F8W) X(F8G) X(F8KS)\n" in form_h and "FORM_BITS = 18" in form_h
