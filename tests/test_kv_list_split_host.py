"""CPU: the split step call on the paged KV cache -- C boundary, Python interface, the unit arithmetic, the build
(include/sage_kvlsplit_gfx950.h, sageattention_amd/_cabi_kvlsplit.py, sageattention_amd/paged_kv_list_split.py, csrc/sage_step_list.h,
csrc/sage_attn_d{128,64}_f8plks.hip, csrc/sage_split_ragged.hip).  The new header's prototypes are the new binding's table and
``sage_kvlist_attn``'s argument list, the library exports them, every argument error of the entry returns -1 with its message before anything
touches a GPU and in the header's order, ``sage_kvlsplit_ws_bytes`` is ``_cabi.kv_split_ws_bytes`` on min(max_seqlen_q, 32) rows, the Python layer
raises ValueError before any work, the unit arithmetic holds over hostile words (a stand-alone program under AddressSanitizer and UBSan), each
new unit holds exactly the list kernels of the seeded packed-group forms, without scratch and at its form's occupancy -- and none of it moved
what the other headers, bindings and units pin."""
import ctypes
import itertools
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import util  # noqa: F401  (sys.path)
import sageattention_amd as sa
import test_build_resources as tbr
import test_kv_list_host as listed_host
import test_kv_step_host as step
import test_kv_varlen_host as varlen
import test_paged_kv_host as paged
from sageattention_amd import _cabi, _cabi_kvcache, _cabi_kvfork, _cabi_kvlist, _cabi_kvlsplit, _cabi_kvpaged, _cabi_kvpool, _cabi_kvpsplit, _cabi_kvpvarlen, _cabi_kvstep
from sageattention_amd.kv_cache import QuantizedKVCache
from sageattention_amd.paged_kv_list_split import sageattn_kvcache_step_split
from test_kv_cache_host import MAIN_HEADER, _prototypes, _text

kf = tbr.kf
ROOT = tbr.ROOT
CSRC = os.path.join(ROOT, "sageattention_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "sage_kvlsplit_gfx950.h")
ENTRIES = ["sage_kvlsplit_abi_version", "sage_kvlsplit_attn", "sage_kvlsplit_ws_bytes"]
_Dev = varlen._Dev


def test_binding_is_the_header_and_the_listed_calls_argument_list():
    protos = _prototypes(HEADER, "SAGE_KVLSPLIT_API")
    assert sorted(protos) == sorted(_cabi_kvlsplit.SYMBOLS) == ENTRIES
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_kvlsplit.SYMBOLS[name]
        assert res is paged._ctype(ret), f"{name}: returns {ret}, bound as {res}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters declared, {len(argtypes)} bound"
        for i, (ctype, bound) in enumerate(zip(params, argtypes)):
            assert bound is paged._ctype(ctype), f"{name}: parameter {i} ({ctype}) bound as {bound}"
    version = int(re.search(r"#define\s+SAGE_KVLSPLIT_ABI_VERSION\s+(\d+)", _text(HEADER)).group(1))
    assert version == 1 == _cabi_kvlsplit.ABI_VERSION
    rest = re.sub(r"SAGE_KVLSPLIT_API", "", _text(HEADER))
    assert "SAGE_API" not in rest and "SAGE_KVLIST_API" not in rest and "SAGE_KVSTEP_API" not in rest          # an export macro of its own
    assert "sage_kvlsplit_gfx950.h" in open(os.path.join(CSRC, "Makefile")).read()
    # the entry takes sage_kvlist_attn's arguments, argument for argument
    theirs = _prototypes(listed_host.HEADER, "SAGE_KVLIST_API")["sage_kvlist_attn"]
    assert protos["sage_kvlsplit_attn"] == theirs
    assert _cabi_kvlsplit.SYMBOLS["sage_kvlsplit_attn"] == _cabi_kvlist.SYMBOLS["sage_kvlist_attn"]


def test_library_exports_the_entries_and_the_other_boundaries_did_not_move():
    lib = ctypes.CDLL(_cabi.LIB_PATH)
    for name in _cabi_kvlsplit.SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
    assert _cabi_kvlsplit.load() is _cabi.load()                     # one library, bound behind _cabi.load()
    assert _cabi_kvlsplit.load().sage_kvlsplit_abi_version() == 1
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22
    assert len(_prototypes(MAIN_HEADER, "SAGE_API")) == 56 and len(_cabi.SYMBOLS) == 56
    assert sorted(_cabi_kvlist.SYMBOLS) == listed_host.ENTRIES and _cabi_kvlist.load().sage_kvlist_abi_version() == 1
    assert sorted(_prototypes(listed_host.HEADER, "SAGE_KVLIST_API")) == listed_host.ENTRIES
    assert sorted(_cabi_kvstep.SYMBOLS) == step.ENTRIES and _cabi_kvstep.load().sage_kvstep_abi_version() == 1
    assert sorted(_cabi_kvpvarlen.SYMBOLS) == varlen.ENTRIES and _cabi_kvpvarlen.load().sage_kvpvarlen_abi_version() == 1
    assert sorted(_cabi_kvpaged.SYMBOLS) == paged.ENTRIES and _cabi_kvpaged.load().sage_kvpaged_abi_version() == 1
    assert _cabi_kvcache.load().sage_kvcache_abi_version() == 1 and _cabi_kvfork.load().sage_kvfork_abi_version() == _cabi_kvfork.ABI_VERSION
    assert _cabi_kvpsplit.load().sage_kvpsplit_abi_version() == _cabi_kvpsplit.ABI_VERSION == 1
    assert _cabi_kvpool.load().sage_kvpool_abi_version() == _cabi_kvpool.ABI_VERSION
    # no symbol starts with another binding's prefix, either way
    bindings = (_cabi, _cabi_kvcache, _cabi_kvpaged, _cabi_kvfork, _cabi_kvpsplit, _cabi_kvpvarlen, _cabi_kvstep, _cabi_kvlist, _cabi_kvpool)
    others = [n for b in bindings for n in b.SYMBOLS]
    assert not any(n.startswith("sage_kvlsplit") for n in others)
    for prefix in ("sage_kvstep", "sage_kvlist", "sage_kvpvarlen", "sage_kvpaged", "sage_kvpsplit", "sage_kvfork", "sage_kvcache", "sage_kvpool"):
        assert not any(n.startswith(prefix) for n in _cabi_kvlsplit.SYMBOLS)
    assert not hasattr(sa, "sageattn_kvcache_step_split") and "sageattn_kvcache_step_split" not in sa.__all__


# ---- argument errors of the entry, in the header's order ------------------------------------------------------------------------------------
_DEFAULT = object()
BIG = 1 << 24


def _attn(lib, p, attr=_DEFAULT, list_ws=_DEFAULT, list_ws_bytes=1 << 20, **kw):
    a = dict(q=p, k_int8=p, v_image=p, o=p, lse=None, k_scale=p, v_scale=p, kv_lens=p, cu_seqlens_q=p, block_table=p, bt_stride=2, num_pages=4,
             page_size=64, max_pages_per_seq=2, B=1, Hq=2, Hkv=1, total_q=1, max_seqlen_q=1, D=64, q_sl=128, q_sh=64, k_sb=4096, k_sh=4096, k_sl=64,
             o_sl=128, o_sh=64, lse_sh=1, is_causal=1, sm_scale_log2=1.0, q_dtype=0, out_dtype=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    if attr is _DEFAULT:
        attr = _cabi.launch_attr(_Dev(p, BIG), kv_split=2, q_start=_Dev(p))
    if list_ws is _DEFAULT:
        list_ws = p
    return lib.sage_kvlsplit_attn(*a.values(), _cabi.attr_arg(attr), list_ws, list_ws_bytes), lib.sage_last_error()


def _raw_attr(p, flags, ws=_DEFAULT, ws_bytes=BIG, window=0):
    """An attribute struct with any flags word (``_cabi.launch_attr`` refuses a chunk count outside [2, 255] itself)."""
    a = _cabi.SageLaunchAttr()
    a.struct_bytes = ctypes.sizeof(_cabi.SageLaunchAttr)
    a.flags = flags
    a.launch_ws = p if ws is _DEFAULT else ws
    a.launch_ws_bytes = ws_bytes
    a.q_start = p
    a.window = window
    return a


def _attn_order(p):
    """sage_kvlist_attn's checks in its order, under this entry's name -- but for its refusal of the split's bit --, then the entry's own four."""
    e = b"sage_kvlsplit_attn: "
    theirs = [(kw, match.replace(b"sage_kvlist_attn: ", e)) for kw, match in listed_host._attn_order(p) if b"SAGE_ATTR_KV_SPLIT is not supported" not in match]
    assert len(theirs) == len(listed_host._attn_order(p)) - 1 and sum(match.startswith(e) for _, match in theirs) == 12
    theirs = [(dict(kw, attr=_cabi.launch_attr(_Dev(p, BIG), kv_split=2, q_start=_Dev(p))) if "attr" in kw else kw, m) for kw, m in theirs]
    S = _cabi.ATTR_KV_SPLIT
    sh = _cabi.ATTR_KV_SPLIT_SHIFT
    return theirs + [(dict(attr=_cabi.launch_attr(q_start=_Dev(p))), e + b"attr must carry SAGE_ATTR_KV_SPLIT"),
                     (dict(attr=_raw_attr(p, S | (1 << sh))), e + b"a chunk count of 2 .. 255 in flags bits 16-23 (got 1)"),
                     (dict(attr=_raw_attr(p, S | (2 << sh), window=5)), e + b"no window with a split (got 5)"),
                     (dict(attr=_raw_attr(p, S | (2 << sh), ws_bytes=128)), e + b"SAGE_ATTR_KV_SPLIT: launch_ws is the split workspace")]


def test_every_argument_error_returns_minus_one_in_the_headers_order():
    lib = _cabi_kvlsplit.load()
    buf, p = paged._aligned_buffer()
    checks = _attn_order(p)
    for kw, match in checks:                                         # each violation alone gives its own message, under the entry's own name
        rc, msg = _attn(lib, p, **kw)
        assert rc == -1 and match in msg and b"sage_kvstep" not in msg and b"sage_kvlist_attn: " not in msg, (kw, rc, msg)
    n = len(checks)
    covered = set()
    for (i, (kw_i, match_i)), (j, (kw_j, _)) in itertools.combinations(enumerate(checks), 2):
        if set(kw_i) & set(kw_j):                                    # two values for one argument do not fit into one call
            continue
        rc, msg = _attn(lib, p, **kw_i, **kw_j)
        assert rc == -1 and match_i in msg, (kw_i, kw_j, rc, msg)
        covered.add((i, j))
    # the last four are four values of one argument, the attributes: each pair of them in one struct, the earlier check's message
    S, sh, e = _cabi.ATTR_KV_SPLIT, _cabi.ATTR_KV_SPLIT_SHIFT, b"sage_kvlsplit_attn: "
    for attr, match in ((_raw_attr(p, 1 << sh, window=5), e + b"attr must carry SAGE_ATTR_KV_SPLIT"),
                        (_raw_attr(p, S | (1 << sh), window=5, ws_bytes=128), e + b"a chunk count of 2 .. 255"),
                        (_raw_attr(p, S, window=5, ws_bytes=128), e + b"a chunk count of 2 .. 255 in flags bits 16-23 (got 0)"),
                        (_raw_attr(p, S | (3 << sh), window=5, ws_bytes=128), e + b"no window with a split"),
                        (_raw_attr(p, S | (3 << sh), ws=None), e + b"SAGE_ATTR_KV_SPLIT: launch_ws is the split workspace"),
                        (_raw_attr(p, S | (3 << sh), ws=p + 64), e + b"SAGE_ATTR_KV_SPLIT: launch_ws is the split workspace")):
        rc, msg = _attn(lib, p, attr=attr)
        assert rc == -1 and match in msg, (rc, msg)
    for i in range(n - 4, n - 1):
        covered.add((i, i + 1))
    # ... and the listed call's last check stands in front of the entry's first
    rc, msg = _attn(lib, p, B=1025, attr=_cabi.launch_attr(q_start=_Dev(p)))
    assert rc == -1 and b"sage_kvlsplit_attn: B must be at most 1024" in msg
    covered.add((n - 5, n - 4))
    assert all((i, i + 1) in covered for i in range(n - 1)), sorted(set((i, i + 1) for i in range(n - 1)) - covered)
    with pytest.raises(ValueError):
        _cabi.check(-1, "sage_kvlsplit_attn")
    # the attributes the listed call refuses by name, under this entry's; the split's bit is the one it takes
    ws, qs = _Dev(p, BIG), _Dev(p)
    for attr, match in ((_cabi.launch_attr(ws, kv_split=2, folded_scores=True, q_start=qs), e + b"SAGE_ATTR_FP8_FOLDED_SCORES is not supported on a paged cache"),
                        (_cabi.launch_attr(ws, kv_split=2, force_persistent=True, q_start=qs), e + b"SAGE_ATTR_FORCE_PERSISTENT is not supported on a paged cache"),
                        (_cabi.launch_attr(ws, kv_split=2, gqa_pack=True, q_start=qs), e + b"SAGE_ATTR_GQA_PACK is not taken (the entry packs the decode rows of a GQA group on its own)"),
                        (_cabi.launch_attr(ws, kv_split=2), e + b"SageLaunchAttr.q_start is required"),
                        (None, e + b"SageLaunchAttr.q_start is required")):
        rc, msg = _attn(lib, p, attr=attr)
        assert rc == -1 and match in msg, (rc, msg)
    # ... and the other entries kept their refusals, under their own names
    rc, msg = listed_host._attn(_cabi_kvlist.load(), p, attr=_cabi.launch_attr(ws, kv_split=2, q_start=qs))
    assert rc == -1 and b"sage_kvlist_attn: SAGE_ATTR_KV_SPLIT is not supported on a paged cache" in msg
    rc, msg = step._attn(_cabi_kvstep.load(), p, attr=_cabi.launch_attr(ws, kv_split=2, q_start=qs))
    assert rc == -1 and b"sage_kvstep_attn: SAGE_ATTR_KV_SPLIT is not supported on a paged cache" in msg
    del buf


def test_ws_bytes_is_the_split_workspace_of_the_decode_rows():
    lib = _cabi_kvlsplit.load()
    for B, Hq, max_q, D, S in ((1, 2, 1, 64, 2), (6, 8, 32, 128, 17), (6, 8, 33, 128, 17), (6, 12, 130, 64, 4), (8, 32, 1, 128, 255), (4, 4, 5, 64, 3),
                               (1024, 64, 2 ** 31 - 1, 128, 255)):
        assert lib.sage_kvlsplit_ws_bytes(B, Hq, max_q, D, S) == _cabi.kv_split_ws_bytes(B, Hq, min(max_q, 32), D, S), (B, Hq, max_q, D, S)
    for bad in ((0, 2, 1, 64, 2), (1, 0, 1, 64, 2), (1, 2, 0, 64, 2), (1, 2, 1, 96, 2), (1, 2, 1, 64, 1), (1, 2, 1, 64, 256), (1, 2, 1, 64, 0), (-1, 2, 1, 64, 2)):
        assert lib.sage_kvlsplit_ws_bytes(*bad) == -1 and b"sage_kvlsplit_ws_bytes" in lib.sage_last_error(), bad


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------------
def test_value_errors_before_any_work():
    c = paged._cache(seeded=True)                # B 2, Hkv 2, D 64, fp16, pages of 128, on the CPU
    q = torch.zeros(5, 4, 64, dtype=torch.float16)
    cu = torch.tensor([0, 2, 5], dtype=torch.int32)
    contiguous = QuantizedKVCache.allocate(2, 2, 64, 64, torch.float16, "cpu")
    for args, kw, match in (
            ((q, contiguous, cu, 3, 2), {}, "sageattn_kvcache_step_split takes a PagedQuantizedKVCache"),
            ((q, "cache", cu, 3, 2), {}, "sageattn_kvcache_step_split takes a PagedQuantizedKVCache"),
            ((q, paged._cache(seeded=False), cu, 3, 2), {}, "no statistics"),
            ((q[:, :2], c, cu, 3, 2), {}, r"sageattn_kvcache_step_split packs the query heads of a GQA group: Hq / Hkv must be at least 2 \(got 2 / 2\)"),
            ((torch.zeros(5, 3, 64, dtype=torch.float16), c, cu, 3, 2), {}, "divisible"),
            ((q.unsqueeze(0), c, cu, 3, 2), {}, "3-D"),
            ((q.float(), c, cu, 3, 2), {}, "dtype"),
            ((q.to("meta"), c, cu, 3, 2), {}, "device"),
            ((q, c, cu, 0, 2), {}, "max_seqlen_q must be a positive int"),
            ((q, c, cu, 3, 256), {}, "sageattn_kvcache_step_split: num_splits must be None, an int in"),
            ((q, c, cu, 3, -1), {}, "sageattn_kvcache_step_split: num_splits must be None, an int in"),
            ((q, c, cu, 3, True), {}, "sageattn_kvcache_step_split: num_splits must be None, an int in"),
            ((q, c, cu, 3, 2.0), {}, "sageattn_kvcache_step_split: num_splits must be None, an int in"),
            ((q, c, cu, 3, "most"), {}, "sageattn_kvcache_step_split: num_splits must be None, an int in"),
            ((q, c, cu.long(), 3, 2), {}, "cu_seqlens_q must be an int32 tensor"),
            ((q, c, cu[:2], 3, 2), {}, r"shape \[B \+ 1\]"),
            ((q, c, cu, 3, 2), dict(q_start=torch.zeros(3, dtype=torch.int32)), r"shape \[B\]"),
            ((q, c, cu, 3, 2), dict(q_start=torch.zeros(2)), "q_start must be an int"),
            # None / 1 / a plan of no split: the listed call's own checks, under its name
            ((q, c, cu.long(), 3, None), {}, "cu_seqlens_q must be an int32 tensor"),
            ((q, c, cu[:2], 3, 1), {}, r"shape \[B \+ 1\]"),
            ((q, c, cu[:2], 3, "auto"), {}, r"shape \[B \+ 1\]"),
            ((q, c, cu[:2], 3, 0), {}, r"shape \[B \+ 1\]")):
        with pytest.raises(ValueError, match=match):
            sageattn_kvcache_step_split(*args, **kw)
    for kw in (dict(window_size=(70, 0)), dict(pack_gqa=True)):
        with pytest.raises(TypeError):
            sageattn_kvcache_step_split(q, c, cu, 3, 2, **kw)
    # the plan is the kv_lens family's, on the decode rows and the logical capacity, packed
    from sageattention_amd import core, paged_kv_list_split as mod
    for B, Hq, Hkv, max_q, cap in ((1, 32, 8, 1, 65536), (4, 32, 8, 512, 32768), (8, 32, 8, 1, 8192), (64, 32, 8, 1, 8192), (1, 32, 8, 1, 4096)):
        assert mod._splits("x", "auto", B, Hq, Hkv, max_q, cap) == mod._splits("x", 0, B, Hq, Hkv, max_q, cap) == core._num_splits_plan(B, Hq, Hkv, min(max_q, 32), cap, True)
    assert mod._splits("x", None, 1, 32, 8, 1, 65536) == mod._splits("x", 1, 1, 32, 8, 1, 65536) == 0 and mod._splits("x", 7, 1, 32, 8, 1, 65536) == 7
    # the modules it stands beside are what they were: it imports their helpers, they know nothing of it
    for name in ("paged_kv_list.py", "paged_kv_step.py", "paged_kv_varlen.py", "paged_kv_split.py"):
        assert "list_split" not in open(os.path.join(ROOT, "sageattention_amd", name)).read()


# ---- the unit arithmetic ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_units_rows_and_tiles_hold_over_hostile_words_under_the_sanitizers(tmp_path):
    """tests/step_split_main.cpp: a program of its own (no GPU, nothing loaded into this process), AddressSanitizer and UBSan on the host."""
    exe = tmp_path / "step_split"
    # (host code only: the file is compiled as C++, every sanitizer option goes to the host compilation by name)
    host = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    out = subprocess.run([tbr.HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", *host, "-I", CSRC,
                          os.path.join(ROOT, "tests", "step_split_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    syms = subprocess.run(["nm", str(exe)], capture_output=True, text=True, timeout=60).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the program was built without the sanitizers"
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    assert run.returncode == 0 and "items each dealt once" in run.stdout and "all inside, none twice" in run.stdout and "runtime error" not in run.stderr and \
        "AddressSanitizer" not in run.stderr, (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    # one definition: the body, pass 1, the merge and the C boundary read the header's functions
    body = open(os.path.join(CSRC, "sage_attn_body.h")).read()
    assert body.count("step_split_item(") == 1 and body.count("if constexpr (LSPLIT)") == 1
    for user, names in (("sage_split_ragged.hip", ("step_split_tile_range(", "step_split_ws_row(", "ragged_band(")),
                        ("sage_merge.hip", ("step_split_ws_row(", "ragged_band(", "merge_split_row<")),
                        ("sage_cabi.hip", ("step_split_ws_rows(", "step_split_grid(", "step_split_tiles("))):
        text = open(os.path.join(CSRC, user)).read()
        assert all(n in text for n in names), user
    # both merge kernels call the one row function
    assert open(os.path.join(CSRC, "sage_merge.hip")).read().count("merge_split_row<") == 2
    # pass 1 of the paged split stands where it stood: the ragged sibling is a translation unit of its own
    assert "ragged" not in open(os.path.join(CSRC, "sage_split_paged.hip")).read()


# ---- the build ------------------------------------------------------------------------------------------------------------------------------
LIST_NAME = listed_host.LIST_NAME


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_split_units_hold_the_seeded_list_kernels_without_scratch_or_hazard():
    import mfma_hazard_lint as lint
    srcs = [f"sage_attn_d{D}_f8plks.hip" for D in (128, 64)]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    in_srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert all(s in in_srcs for s in srcs) and "sage_split_ragged.hip" in in_srcs
    # the lint's new tuple names them and is disjoint from the others, whose contents stand
    assert lint.UNITS_PAGED_LIST_SPLIT == tuple(srcs)
    rest = (lint.UNITS + lint.UNITS_PAIR + lint.UNITS_WINDOW + lint.UNITS_PACKED_BR + lint.UNITS_PACKED_WINDOW + lint.UNITS_GQA_PACK + lint.UNITS_KV_SPLIT +
            lint.UNITS_PAGED + lint.UNITS_PAGED_SPLIT + lint.UNITS_PAGED_RAGGED + lint.UNITS_PAGED_STEP + lint.UNITS_PAGED_LIST)
    assert not set(srcs) & set(rest) and len(rest) == 40
    assert lint.UNITS_PAGED_LIST == ("sage_attn_d128_f8pl.hip", "sage_attn_d64_f8pl.hip", "sage_attn_d128_f8plg.hip", "sage_attn_d64_f8plg.hip")
    with ThreadPoolExecutor(max_workers=5) as ex:
        reports = ex.map(tbr._resource_report, srcs + ["sage_split_ragged.hip"])
        lints = ex.map(lambda u: lint.lint(lint.listing(u)), srcs)
        reports, lints = dict(zip(srcs + ["sage_split_ragged.hip"], reports)), dict(zip(srcs, lints))
    for D in (128, 64):
        src = f"sage_attn_d{D}_f8plks.hip"
        rep = reports[src]
        # the QSTART + GPACK forms of the kv_lens split's list: two of its eight (fp16 / bf16 q), the words the paged split's units hold as well
        theirs = tbr._resource_report(f"sage_attn_d{D}_f8pks.hip")
        every = [int(re.search(r"ILj(\d+)E", k).group(1)) for k in theirs]
        want = {w: (3 if D == 64 else 2) for w in every if kf.unpack(w)["qstart"] and kf.unpack(w)["gpack"]}
        assert len(want) == 2 and len(every) == 8
        assert len(rep) == 2, sorted(rep)
        for name, res in rep.items():
            m = re.fullmatch(LIST_NAME, name)
            assert m, name                                             # (the list entry, and no kernel of another entry)
            word = int(m.group(1))
            f = kf.unpack(word)
            assert word in want and f["D"] == D and f["causal"] and f["qstart"] and f["kvlen"] and f["pv_fp8"] and f["seed"] and f["gpack"] and not f["window"], (name, f)
            assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0 and res.get("SGPRs Spill", 0) == 0, (name, res)
            assert res["Occupancy"] >= want[word] == (3 if D == 64 else 2), (name, res)          # the form's own bound: no two-wave fallback
        assert {int(re.fullmatch(LIST_NAME, k).group(1)) for k in rep} == set(want) and {kf.unpack(w)["qf"] for w in want} == {1, 2}
        findings, n_mfma = lints[src]
        assert n_mfma >= 50 and not findings, (src, n_mfma, findings[:5])
    p1 = reports["sage_split_ragged.hip"]
    assert len(p1) == 4 and all("chunk_max_lens_ragged_kernel" in k for k in p1), sorted(p1)
    assert all(res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0 for res in p1.values())
    # the listed units hold what they held, and the form table is untouched: no form bit, no member of the unit list
    for D in (128, 64):
        for u in ("f8pl", "f8plg", "f8pks"):
            text = open(os.path.join(CSRC, f"sage_attn_d{D}_{u}.hip")).read()
            assert "lsplit" not in text
    form_h = open(os.path.join(CSRC, "sage_attn_form.h")).read()
    assert "X(F8) X(F8F) X(F16) X(F8V) X(F8VB) X(F8VBW) X(F8S) X(F8K) X(F8Q) X(F8W) X(F8G) X(F8KS)\n" in form_h and "FORM_BITS = 18" in form_h
