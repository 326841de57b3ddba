"""CPU: the packed, variable-length calls on the paged KV cache -- C boundary, Python interface, the clamp, the build
(include/sage_kvpvarlen_gfx950.h, sageattention_amd/_cabi_kvpvarlen.py, sageattention_amd/paged_kv_varlen.py, csrc/sage_ragged.h,
csrc/sage_attn_d{128,64}_f8pr.hip, csrc/sage_kv_varlen.hip).  The new header's prototypes are the new binding's table, the library exports
them, every argument error of the two entries returns -1 with its message before anything touches a GPU and in the header's order, the
Python layer raises ValueError before any work, the clamp between a prefix array and every address holds over hostile words (a stand-alone
program under AddressSanitizer and UBSan), each new unit holds exactly the ragged kernels of the forms it is instantiated from, without
scratch and at its form's occupancy -- and none of it moved what the other headers and bindings pin."""
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
import test_paged_kv_host as paged
from sageattention_amd import _cabi, _cabi_kvcache, _cabi_kvfork, _cabi_kvpaged, _cabi_kvpsplit, _cabi_kvpvarlen
from sageattention_amd.kv_cache import QuantizedKVCache
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
from sageattention_amd.paged_kv_varlen import append_varlen, sageattn_kvcache_varlen
from test_kv_cache_host import MAIN_HEADER, _prototypes, _text
from test_paged_kv_host import listed  # noqa: F401  (the fixture: the forms of the lists the paged and the ragged units are instantiated from)

kf = tbr.kf
ROOT = tbr.ROOT
CSRC = os.path.join(ROOT, "sageattention_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "sage_kvpvarlen_gfx950.h")
ENTRIES = ["sage_kvpvarlen_abi_version", "sage_kvpvarlen_append", "sage_kvpvarlen_attn"]


def test_binding_is_the_header():
    protos = _prototypes(HEADER, "SAGE_KVPVARLEN_API")
    assert sorted(protos) == sorted(_cabi_kvpvarlen.SYMBOLS) == ENTRIES
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_kvpvarlen.SYMBOLS[name]
        assert res is paged._ctype(ret), f"{name}: returns {ret}, bound as {res}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters declared, {len(argtypes)} bound"
        for i, (ctype, bound) in enumerate(zip(params, argtypes)):
            assert bound is paged._ctype(ctype), f"{name}: parameter {i} ({ctype}) bound as {bound}"
    version = int(re.search(r"#define\s+SAGE_KVPVARLEN_ABI_VERSION\s+(\d+)", _text(HEADER)).group(1))
    assert version == 1 == _cabi_kvpvarlen.ABI_VERSION
    rest = re.sub(r"SAGE_KVPVARLEN_API", "", _text(HEADER))
    assert "SAGE_API" not in rest and "SAGE_KVPAGED_API" not in rest          # an export macro of its own
    assert "sage_kvpvarlen_gfx950.h" in open(os.path.join(CSRC, "Makefile")).read()


def test_library_exports_the_entries_and_the_other_boundaries_did_not_move():
    lib = ctypes.CDLL(_cabi.LIB_PATH)
    for name in _cabi_kvpvarlen.SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
    assert _cabi_kvpvarlen.load() is _cabi.load()                    # one library, bound behind _cabi.load()
    assert _cabi_kvpvarlen.load().sage_kvpvarlen_abi_version() == 1
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22
    assert len(_prototypes(MAIN_HEADER, "SAGE_API")) == 56 and len(_cabi.SYMBOLS) == 56
    assert sorted(_cabi_kvpaged.SYMBOLS) == paged.ENTRIES and _cabi_kvpaged.load().sage_kvpaged_abi_version() == 1
    assert _cabi_kvcache.load().sage_kvcache_abi_version() == 1 and _cabi_kvfork.load().sage_kvfork_abi_version() == _cabi_kvfork.ABI_VERSION
    assert _cabi_kvpsplit.load().sage_kvpsplit_abi_version() == _cabi_kvpsplit.ABI_VERSION
    others = [n for b in (_cabi, _cabi_kvcache, _cabi_kvpaged, _cabi_kvfork, _cabi_kvpsplit) for n in b.SYMBOLS]
    assert not any(n.startswith("sage_kvpvarlen") for n in others)
    assert not any(hasattr(sa, n) for n in ("sageattn_kvcache_varlen", "append_varlen")) and "sageattn_kvcache_varlen" not in sa.__all__


# ---- argument errors of the two entries, in the header's order ---------------------------------------------------------------------------
class _Dev:
    """What ``_cabi.launch_attr`` asks of a tensor, at a host address (no call here reaches a launch)."""

    def __init__(self, p, n=4096):
        self.p, self.n = p, n

    def data_ptr(self):
        return self.p

    def numel(self):
        return self.n

    def element_size(self):
        return 1


def _append(lib, p, **kw):
    a = dict(k_int8=p, k_scale=p, v_image=p, v_scale=p, v_amax=p, k_mean=None, k_tail=p, v_tail=p, lens=p, k_new=p, v_new=p, cu_seqlens=p,
             B=1, Hkv=1, total=1, max_new=1, head_dim=64, k_sl=64, k_sh=64, v_sl=64, v_sh=64, dtype=0,
             block_table=p, bt_stride=2, num_pages=4, page_size=64, max_pages_per_seq=2, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.sage_kvpvarlen_append(*a.values()), lib.sage_last_error()


_DEFAULT = object()


def _attn(lib, p, attr=_DEFAULT, **kw):
    a = dict(q=p, k_int8=p, v_image=p, o=p, lse=None, k_scale=p, v_scale=p, kv_lens=p, cu_seqlens_q=p, block_table=p, bt_stride=2, num_pages=4,
             page_size=64, max_pages_per_seq=2, B=1, Hq=2, Hkv=1, total_q=1, max_seqlen_q=1, D=64, q_sl=128, q_sh=64, k_sb=4096, k_sh=4096, k_sl=64,
             o_sl=128, o_sh=64, lse_sh=1, is_causal=1, sm_scale_log2=1.0, q_dtype=0, out_dtype=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    if attr is _DEFAULT:
        attr = _cabi.launch_attr(q_start=_Dev(p))
    return lib.sage_kvpvarlen_attn(*a.values(), _cabi.attr_arg(attr)), lib.sage_last_error()


def _append_order(p):
    return [(dict(k_int8=None), b"null cache pointer"),
            (dict(k_new=None), b"null k_new / v_new"),
            (dict(cu_seqlens=None), b"null cu_seqlens"),
            (dict(block_table=None), b"null block_table"),
            (dict(page_size=96), b"page_size must be 64 * 2^k"),
            (dict(num_pages=0), b"num_pages must be at least 1"),
            (dict(max_pages_per_seq=0), b"max_pages_per_seq must be at least 1"),
            (dict(B=0), b"B and Hkv"),
            (dict(head_dim=96), b"head_dim must be 64 or 128"),
            (dict(max_new=0), b"T must be at least 1"),
            (dict(total=0), b"total must be at least 1"),
            (dict(dtype=2), b"bad dtype"),
            (dict(v_image=p + 2), b"16-byte aligned"),
            (dict(block_table=p + 2), b"block_table must be 4-byte aligned"),
            (dict(cu_seqlens=p + 2), b"cu_seqlens must be 4-byte aligned"),
            (dict(k_sl=68), b"multiples of 8 elements")]


def _attn_order(p):
    return [(dict(q=None), b"null tensor pointer"),
            (dict(kv_lens=None), b"null kv_lens"),
            (dict(cu_seqlens_q=None), b"null cu_seqlens_q"),
            (dict(block_table=None), b"null block_table"),
            (dict(page_size=96), b"page_size must be 64 * 2^k"),
            (dict(num_pages=0), b"num_pages must be at least 1"),
            (dict(max_pages_per_seq=0), b"max_pages_per_seq must be at least 1"),
            (dict(B=0), b"B and Hkv"),
            (dict(block_table=p + 2), b"block_table must be 4-byte aligned"),
            (dict(cu_seqlens_q=p + 2), b"cu_seqlens_q must be 4-byte aligned"),
            (dict(total_q=0), b"total_q and max_seqlen_q must be at least 1"),
            (dict(is_causal=0), b"is_causal must be 1"),
            (dict(Hq=2 ** 20, max_seqlen_q=2 ** 20), b"must be in [1, 2^31)"),
            (dict(lse=p, lse_sh=0), b"lse_sh must be at least total_q"),
            (dict(attr=_cabi.launch_attr(folded_scores=True, q_start=_Dev(p))), b"sage_kvpvarlen_attn: SAGE_ATTR_FP8_FOLDED_SCORES is not supported on a paged cache"),
            (dict(D=96), b"head_dim must be 64 or 128"),
            (dict(Hkv=3), b"divisible"),
            (dict(q_dtype=2), b"bad q_dtype"),
            (dict(out_dtype=-1), b"bad out_dtype"),
            (dict(o=p + 2), b"16-byte aligned"),
            (dict(q_sl=68), b"q strides"),
            (dict(k_sl=72), b"k strides"),
            (dict(o_sh=4), b"output strides")]


ORDERS = {"sage_kvpvarlen_append": (_append, _append_order), "sage_kvpvarlen_attn": (_attn, _attn_order)}


@pytest.mark.parametrize("entry", sorted(ORDERS))
def test_every_argument_error_returns_minus_one_in_the_headers_order(entry):
    call, order = ORDERS[entry]
    lib = _cabi_kvpvarlen.load()
    buf, p = paged._aligned_buffer()
    checks = order(p)
    for kw, match in checks:                                         # each violation alone gives its own message
        rc, msg = call(lib, p, **kw)
        assert rc == -1 and match in msg, (entry, kw, rc, msg)
    covered = set()
    for (i, (kw_i, match_i)), (j, (kw_j, _)) in itertools.combinations(enumerate(checks), 2):
        if set(kw_i) & set(kw_j):                                    # two values for one argument do not fit into one call
            continue
        rc, msg = call(lib, p, **kw_i, **kw_j)
        assert rc == -1 and match_i in msg, (entry, kw_i, kw_j, rc, msg)
        covered.add((i, j))
    assert all((i, i + 1) in covered for i in range(len(checks) - 1)), (entry, sorted(covered))
    with pytest.raises(ValueError):
        _cabi.check(-1, entry)
    del buf


def test_attention_refuses_by_name_what_the_paged_entry_refuses():
    lib = _cabi_kvpvarlen.load()
    buf, p = paged._aligned_buffer()
    ws, qs = _Dev(p), _Dev(p)
    e = b"sage_kvpvarlen_attn: "
    for attr, match in ((_cabi.launch_attr(ws, kv_split=2, q_start=qs), e + b"SAGE_ATTR_KV_SPLIT is not supported on a paged cache"),
                        (_cabi.launch_attr(folded_scores=True, q_start=qs), e + b"SAGE_ATTR_FP8_FOLDED_SCORES is not supported on a paged cache"),
                        (_cabi.launch_attr(ws, force_persistent=True, q_start=qs), e + b"SAGE_ATTR_FORCE_PERSISTENT is not supported on a paged cache"),
                        (_cabi.launch_attr(gqa_pack=True, q_start=qs), e + b"SAGE_ATTR_GQA_PACK is not supported on packed query rows"),
                        # ... in that order, and all of them in front of the missing offsets
                        (_cabi.launch_attr(folded_scores=True, gqa_pack=True), e + b"SAGE_ATTR_FP8_FOLDED_SCORES"),
                        (_cabi.launch_attr(gqa_pack=True), e + b"SAGE_ATTR_GQA_PACK"),
                        (_cabi.launch_attr(window=5), e + b"SageLaunchAttr.q_start is required"),
                        (None, e + b"SageLaunchAttr.q_start is required")):
        rc, msg = _attn(lib, p, attr=attr)
        assert rc == -1 and match in msg, (rc, msg)
    # the paged entry's own messages kept their wording
    rc, msg = paged._attn(_cabi_kvpaged.load(), p, attr=_cabi.launch_attr(folded_scores=True))
    assert rc == -1 and b"sage_kvpaged_attn: SAGE_ATTR_FP8_FOLDED_SCORES is not supported on a paged cache (the exact score form only)" in msg
    del buf


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
def _cache(seeded=True):
    return paged._cache(seeded=seeded)           # B 2, Hkv 2, D 64, fp16, pages of 128, on the CPU


def test_attention_value_errors_before_any_work():
    c = _cache()
    q = torch.zeros(5, 4, 64, dtype=torch.float16)
    cu = torch.tensor([0, 2, 5], dtype=torch.int32)
    contiguous = QuantizedKVCache.allocate(2, 2, 64, 64, torch.float16, "cpu")
    for args, kw, match in (
            ((q, contiguous, cu, 3), {}, "takes a PagedQuantizedKVCache"),
            ((q, "cache", cu, 3), {}, "takes a PagedQuantizedKVCache"),
            ((q, _cache(seeded=False), cu, 3), {}, "no statistics"),
            ((q, c, cu, 3), dict(pack_gqa=True), "pack_gqa is not supported by sageattn_kvcache_varlen"),
            ((q, c, cu, 3), dict(num_splits=2), "num_splits is not supported by sageattn_kvcache_varlen"),
            ((q, c, cu, 3), dict(num_splits="auto"), "num_splits is not supported by sageattn_kvcache_varlen"),
            ((q.unsqueeze(0), c, cu, 3), {}, "3-D"),
            ((q.float(), c, cu, 3), {}, "dtype"),
            ((q.to("meta"), c, cu, 3), {}, "device"),
            ((torch.zeros(5, 4, 128, dtype=torch.float16), c, cu, 3), {}, "must be"),
            ((torch.zeros(0, 4, 64, dtype=torch.float16), c, cu, 3), {}, "must be"),
            ((torch.zeros(5, 3, 64, dtype=torch.float16), c, cu, 3), {}, "divisible"),
            ((q, c, cu.long(), 3), {}, "cu_seqlens_q must be an int32 tensor"),
            ((q, c, [0, 2, 5], 3), {}, "cu_seqlens_q must be an int32 tensor"),
            ((q, c, cu[:2], 3), {}, r"shape \[B \+ 1\]"),
            ((q, c, cu.to("meta"), 3), {}, "device"),
            ((q, c, cu, 0), {}, "max_seqlen_q must be a positive int"),
            ((q, c, cu, True), {}, "max_seqlen_q must be a positive int"),
            ((q, c, cu, torch.tensor(3)), {}, "max_seqlen_q must be a positive int"),
            # the keywords that exist on the dense call: the family's one resolver, its messages
            ((q, c, cu, 3), dict(window_size=(70,)), "window_size"),
            ((q, c, cu, 3), dict(window_size=(70, 5)), "window_size"),
            ((q, c, cu, 3), dict(q_start=torch.zeros(3, dtype=torch.int32)), r"shape \[B\]"),
            ((q, c, cu, 3), dict(q_start=torch.zeros(2)), "q_start must be an int")):
        with pytest.raises(ValueError, match=match):
            sageattn_kvcache_varlen(*args, **kw)


def test_append_value_errors_before_any_work():
    c = _cache()
    h = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt)
    cu = torch.tensor([0, 2, 5], dtype=torch.int32)
    contiguous = QuantizedKVCache.allocate(2, 2, 64, 64, torch.float16, "cpu")
    for args, match in (
            ((contiguous, h(5, 2, 64), h(5, 2, 64), cu, 3), "takes a PagedQuantizedKVCache"),
            ((_cache(seeded=False), h(5, 2, 64), h(5, 2, 64), cu, 3), "no statistics"),
            ((c, h(2, 2, 3, 64), h(2, 2, 3, 64), cu, 3), "3-D"),
            ((c, h(5, 2, 64, dt=torch.bfloat16), h(5, 2, 64, dt=torch.bfloat16), cu, 3), "dtype"),
            ((c, h(5, 4, 64), h(5, 4, 64), cu, 3), "must be"),
            ((c, h(5, 2, 128), h(5, 2, 128), cu, 3), "must be"),
            ((c, h(5, 2, 64), h(6, 2, 64), cu, 3), "one shape"),
            ((c, h(5, 2, 64), h(5, 2, 64), cu.long(), 3), "cu_seqlens must be an int32 tensor"),
            ((c, h(5, 2, 64), h(5, 2, 64), cu[:1], 3), r"shape \[B \+ 1\]"),
            ((c, h(5, 2, 64), h(5, 2, 64), cu, 0), "max_new must be a positive int"),
            ((c, h(5, 2, 64), h(5, 2, 64), cu, 2.0), "max_new must be a positive int")):
        with pytest.raises(ValueError, match=match):
            append_varlen(*args)
    assert c.lens.tolist() == [0, 0]
    assert not hasattr(PagedQuantizedKVCache, "append_varlen")      # a function of its module: the classes are what they were


# ---- the clamp --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_clamp_holds_over_hostile_prefix_words_under_the_sanitizers(tmp_path):
    """tests/ragged_clamp_main.cpp: a program of its own (no GPU, nothing loaded into this process), AddressSanitizer and UBSan on the host."""
    exe = tmp_path / "ragged_clamp"
    # (host code only: every sanitizer option goes to the host compilation by name, none reaches a device code object)
    host = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    out = subprocess.run([tbr.HIPCC, "-std=c++17", "-O1", "-g", *host, "-I", CSRC,
                          os.path.join(ROOT, "tests", "ragged_clamp_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    syms = subprocess.run(["nm", str(exe)], capture_output=True, text=True, timeout=60).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the program was built without the sanitizers"
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "all inside" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, \
        (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    # the kernels and the program read one definition
    assert '#include "sage_ragged.h"' in open(os.path.join(CSRC, "sage_attn_kernel.h")).read()
    assert '#include "sage_ragged.h"' in open(os.path.join(CSRC, "sage_kv_varlen.hip")).read()
    body = open(os.path.join(CSRC, "sage_attn_body.h")).read()
    assert body.count("ragged_rows(") == 2 and "ragged_rows(" in open(os.path.join(CSRC, "sage_kv_varlen.hip")).read()


# ---- the build --------------------------------------------------------------------------------------------------------------------------
RAGGED_UNITS = ("UNIT_F8Q", "UNIT_F8W")


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_ragged_units_hold_the_ragged_kernels_of_their_lists_without_scratch(listed):  # noqa: F811
    srcs = ["sage_attn_d128_f8pr.hip", "sage_attn_d64_f8pr.hip", "sage_kv_varlen.hip"]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert all(s in re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split() for s in srcs)
    with ThreadPoolExecutor(max_workers=len(srcs)) as ex:
        reports = dict(zip(srcs, ex.map(tbr._resource_report, srcs)))
    for D in (128, 64):
        rep = reports[f"sage_attn_d{D}_f8pr.hip"]
        want = {}
        for unit in RAGGED_UNITS:
            want.update(listed[(unit, D)])
        assert len(want) == 4                       # causal, q_start, kv_lens, with and without a window, fp16 and bf16 q
        assert not [k for k in rep if "sage_attn_kernel" in k or "sage_attn_paged_kernel" in k], "a kernel of another family in a ragged unit"
        mine = {k: v for k, v in rep.items() if "sage_attn_paged_varlen_kernel" in k}
        assert len(mine) == 4 and len(rep) == 4, sorted(rep)
        for name, res in mine.items():
            m = re.fullmatch(r"_ZN4sage29sage_attn_paged_varlen_kernelILj(\d+)EEEvNS_10AttnParamsENS_9PagedArgsENS_10RaggedArgsE", name)
            assert m, name
            word = int(m.group(1))
            f = kf.unpack(word)
            assert word in want and f["D"] == D and f["causal"] and f["qstart"] and f["kvlen"] and f["pv_fp8"] and not f["seed"] and not f["gpack"], (name, f)
            assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0, (name, res)
            assert res["Occupancy"] >= want[word] == (3 if D == 64 else 2), (name, res)          # the form's own bound: no two-wave fallback
        assert {int(re.search(r"ILj(\d+)E", k).group(1)) for k in mine} == set(want)
    rep = reports["sage_kv_varlen.hip"]
    assert len(rep) == 5 and sum("kvpvarlen_append_kernel" in k for k in rep) == 4 and sum("kvpvarlen_commit_kernel" in k for k in rep) == 1, sorted(rep)
    for name, res in rep.items():
        assert res.get("ScratchSize", 0) == 0 and res.get("VGPRs Spill", 0) == 0, (name, res)
    # the existing cache units hold what they held (kernels added there renumber the registers of those already there)
    for src, n in (("sage_kv_cache.hip", 5), ("sage_kv_paged.hip", 4)):
        text = open(os.path.join(CSRC, src)).read()
        assert "RaggedArgs" not in text and "ragged" not in text.lower(), src
