"""CPU: the exact split-KV call on the paged KV cache -- its C boundary, Python interface and build (include/sage_kvpsplit_gfx950.h,
sageattention_amd/_cabi_kvpsplit.py, sageattention_amd/paged_kv_split.py, csrc/sage_attn_d{128,64}_f8pks.hip, csrc/sage_split_paged.hip; DESIGN
3.20).  The new header's prototypes are the new binding's table, the library exports them, every argument error of ``sage_kvpsplit_attn`` returns
-1 with a message that names the entry before anything touches a GPU and in the documented order, the Python name raises the family's
ValueErrors before any work, the two new attention units hold exactly the paged kernels of ``unit_forms(UNIT_F8KS, D)`` without scratch or
spills at the occupancy of their forms, the lint walks them without a finding -- and none of it moved what the four older headers, their
bindings and ``sageattn_kvcache`` pin.  Last, which table entries a paged split call may read, restated in numpy from
``loop_plan.split_chunk`` and held against cases written out by hand."""
import ctypes
import itertools
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import util  # noqa: F401  (sys.path)
import loop_plan as lp
import sageattention_amd as sa
import test_build_resources as tbr
import test_paged_kv_host as paged
from sageattention_amd import _cabi, _cabi_kvcache, _cabi_kvfork, _cabi_kvpaged, _cabi_kvpsplit
from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
from sageattention_amd.paged_kv_split import sageattn_kvcache_split
from test_kv_cache_host import MAIN_HEADER, _prototypes, _text

kf = tbr.kf
ROOT = tbr.ROOT
CSRC = os.path.join(ROOT, "sageattention_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "sage_kvpsplit_gfx950.h")
ENTRIES = ["sage_kvpsplit_abi_version", "sage_kvpsplit_attn"]
E = b"sage_kvpsplit_attn"


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------
def test_binding_is_the_header():
    protos = _prototypes(HEADER, "SAGE_KVPSPLIT_API")
    assert sorted(protos) == sorted(_cabi_kvpsplit.SYMBOLS) == ENTRIES
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_kvpsplit.SYMBOLS[name]
        assert res is paged._ctype(ret), f"{name}: returns {ret}, bound as {res}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters declared, {len(argtypes)} bound"
        for i, (ctype, bound) in enumerate(zip(params, argtypes)):
            assert bound is paged._ctype(ctype), f"{name}: parameter {i} ({ctype}) bound as {bound}"
    version = int(re.search(r"#define\s+SAGE_KVPSPLIT_ABI_VERSION\s+(\d+)", _text(HEADER)).group(1))
    assert version == 1 == _cabi_kvpsplit.ABI_VERSION
    rest = re.sub(r"SAGE_KVPSPLIT_API", "", _text(HEADER))
    assert not re.search(r"\bSAGE_API\b|SAGE_KVCACHE_API|SAGE_KVPAGED_API|SAGE_KVFORK_API", rest)          # an export macro of its own
    # sage_kvpaged_attn's argument list, argument for argument
    theirs = _prototypes(os.path.join(ROOT, "include", "sage_kvpaged_gfx950.h"), "SAGE_KVPAGED_API")["sage_kvpaged_attn"]
    assert protos["sage_kvpsplit_attn"] == theirs
    assert _cabi_kvpsplit.SYMBOLS["sage_kvpsplit_attn"] == _cabi_kvpaged.SYMBOLS["sage_kvpaged_attn"]


def test_library_exports_the_entries():
    lib = ctypes.CDLL(_cabi.LIB_PATH)
    for name in _cabi_kvpsplit.SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
    assert _cabi_kvpsplit.load() is _cabi.load()                     # one library, bound behind _cabi.load()
    assert _cabi_kvpsplit.load().sage_kvpsplit_abi_version() == 1


def test_the_four_older_boundaries_did_not_move():
    lib = _cabi.load()
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22
    assert len(_prototypes(MAIN_HEADER, "SAGE_API")) == 56 and len(_cabi.SYMBOLS) == 56
    inc = lambda h: os.path.join(ROOT, "include", h)
    assert sorted(_prototypes(inc("sage_kvcache_gfx950.h"), "SAGE_KVCACHE_API")) == sorted(_cabi_kvcache.SYMBOLS) == ["sage_kvcache_abi_version", "sage_kvcache_append"]
    assert sorted(_prototypes(inc("sage_kvpaged_gfx950.h"), "SAGE_KVPAGED_API")) == sorted(_cabi_kvpaged.SYMBOLS) == paged.ENTRIES
    assert sorted(_prototypes(inc("sage_kvfork_gfx950.h"), "SAGE_KVFORK_API")) == sorted(_cabi_kvfork.SYMBOLS) == ["sage_kvfork", "sage_kvfork_abi_version"]
    for binding, sym in ((_cabi_kvcache, "sage_kvcache_abi_version"), (_cabi_kvpaged, "sage_kvpaged_abi_version"), (_cabi_kvfork, "sage_kvfork_abi_version")):
        assert binding.ABI_VERSION == 1 and getattr(binding.load(), sym)() == 1
    for table in (_cabi.SYMBOLS, _cabi_kvcache.SYMBOLS, _cabi_kvpaged.SYMBOLS, _cabi_kvfork.SYMBOLS):
        assert not any(n.startswith("sage_kvpsplit") for n in table)
    assert "sage_kvpsplit_gfx950.h" in open(inc("sage_kvpaged_gfx950.h")).read() and "kvpsplit" not in _text(inc("sage_kvpaged_gfx950.h"))      # (a pointer in a comment, nothing else)
    assert sorted(sa.__all__) == sorted(["sageattn", "sageattn_varlen", "sageattn_qk_int8_pv_fp16_triton", "sageattn_qk_int8_pv_fp16_cuda",
                                         "sageattn_qk_int8_pv_fp8_cuda", "sageattn_qk_int8_pv_fp8_cuda_sm90", "sageattn_qk_int8_pv_fp8_varlen"])
    assert not hasattr(sa, "sageattn_kvcache_split")


# ---- argument errors of sage_kvpsplit_attn --------------------------------------------------------------------------------------------
class _Ws:
    """What ``_cabi.launch_attr`` asks of a workspace tensor, over host memory (the library must refuse before its first HIP call)."""
    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.nbytes

    def element_size(self):
        return 1


NEED = _cabi.kv_split_ws_bytes(1, 2, 1, 64, 4)          # of the default call below with S = 4


def _attr(p, S=4, nbytes=1 << 30, **kw):
    return _cabi.launch_attr(_Ws(p, nbytes), kv_split=S, **kw)


def _raw_attr(flags, p=None, nbytes=0, window=0):
    return _cabi.SageLaunchAttr(struct_bytes=ctypes.sizeof(_cabi.SageLaunchAttr), flags=flags, launch_ws=p, launch_ws_bytes=nbytes, window=window)


def _attn(lib, p, attr="default", **kw):
    a = dict(q=p, k_int8=p, v_image=p, o=p, lse=None, k_scale=p, v_scale=p, kv_lens=p, block_table=p, bt_stride=2, num_pages=4, page_size=64,
             max_pages_per_seq=2, B=1, Hq=2, Hkv=1, Lq=1, D=64, q_sb=128, q_sh=64, q_sl=64, k_sb=4096, k_sh=4096, k_sl=64, o_sb=128, o_sh=64, o_sl=64,
             is_causal=0, sm_scale_log2=1.0, q_dtype=0, out_dtype=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    attr = _attr(p) if isinstance(attr, str) else attr
    return lib.sage_kvpsplit_attn(*a.values(), _cabi.attr_arg(attr)), lib.sage_last_error()


def _order(p):
    """One violation per check, in the order the entry checks."""
    split = _cabi.ATTR_KV_SPLIT
    count = lambda S: S << _cabi.ATTR_KV_SPLIT_SHIFT
    return [(dict(q=None), b"null tensor pointer"),
            (dict(kv_lens=None), b"null kv_lens"),
            (dict(block_table=None), b"null block_table"),
            (dict(page_size=96), b"page_size must be 64 * 2^k"),
            (dict(num_pages=0), b"num_pages must be at least 1"),
            (dict(max_pages_per_seq=0), b"max_pages_per_seq must be at least 1"),
            (dict(B=0), b"B and Hkv"),
            (dict(block_table=p + 2), b"block_table must be 4-byte aligned"),
            (dict(attr=None), b"attr must carry SAGE_ATTR_KV_SPLIT"),
            (dict(attr=_raw_attr(split | count(1), p, 1 << 30)), b"a chunk count of 2 .. 255"),
            (dict(Lq=129), b"Lq <= 128"),
            (dict(attr=_raw_attr(split | count(4), p, 1 << 30, window=7)), b"no window with a split"),
            (dict(attr=_raw_attr(split | count(4) | _cabi.ATTR_FP8_FOLDED_SCORES, p, 1 << 30)), b"SAGE_ATTR_FP8_FOLDED_SCORES is not supported"),
            (dict(attr=_raw_attr(split | count(4) | _cabi.ATTR_FORCE_PERSISTENT, p, 1 << 30)), b"SAGE_ATTR_FORCE_PERSISTENT is not supported"),
            (dict(attr=_raw_attr(split | count(4), p, NEED - 1)), b"split workspace"),
            (dict(D=96), b"head_dim must be 64 or 128"),
            (dict(Hq=3, Hkv=2), b"divisible"),
            (dict(q_dtype=2), b"bad q_dtype"),
            (dict(out_dtype=-1), b"bad out_dtype"),
            (dict(o=p + 2), b"16-byte aligned"),
            (dict(q_sl=68), b"q strides"),
            (dict(k_sl=72), b"k strides"),
            (dict(o_sh=4), b"output strides")]


def test_argument_errors_do_not_need_a_gpu():
    lib = _cabi_kvpsplit.load()
    buf, p = paged._aligned_buffer()
    for name in ("q", "k_int8", "v_image", "o", "k_scale", "v_scale"):
        rc, msg = _attn(lib, p, **{name: None})
        assert rc == -1 and E in msg and b"null tensor pointer" in msg, (name, rc, msg)
    # the page geometry through paged_args, as sage_kvpaged_attn
    for ps in paged.BAD_PAGE_SIZES:
        rc, msg = _attn(lib, p, page_size=ps)
        assert rc == -1 and E in msg and b"page_size must be 64 * 2^k" in msg, (ps, msg)
    for kw in (dict(max_pages_per_seq=0), dict(page_size=2 ** 30, max_pages_per_seq=2), dict(bt_stride=1)):
        rc, msg = _attn(lib, p, **kw)
        assert rc == -1 and E in msg and b"max_pages_per_seq must be at least 1" in msg, (kw, msg)
    for kw in (dict(B=0), dict(B=65536), dict(Hkv=0), dict(Hkv=65536)):
        rc, msg = _attn(lib, p, **kw)
        assert rc == -1 and E in msg and b"B and Hkv" in msg, (kw, msg)
    # a missing flag: no attributes, attributes without the bit, a count without the bit
    for attr in (None, _cabi.launch_attr(gqa_pack=True), _raw_attr(4 << 16, p, 1 << 30), _raw_attr(0, p, 1 << 30)):
        rc, msg = _attn(lib, p, attr=attr)
        assert rc == -1 and E + b": attr must carry SAGE_ATTR_KV_SPLIT" in msg, (rc, msg)
    # S outside [2, 255] (the eight count bits hold no more)
    for S in (0, 1):
        rc, msg = _attn(lib, p, attr=_raw_attr(_cabi.ATTR_KV_SPLIT | (S << 16), p, 1 << 30))
        assert rc == -1 and E in msg and b"2 .. 255" in msg and f"got {S}".encode() in msg, (S, msg)
    for Lq in (129, 4096):
        rc, msg = _attn(lib, p, Lq=Lq)
        assert rc == -1 and E in msg and b"Lq <= 128" in msg, (Lq, msg)
    rc, msg = _attn(lib, p, attr=_attr(p, window=100), is_causal=1)
    assert rc == -1 and E in msg and b"no window" in msg, msg
    rc, msg = _attn(lib, p, attr=_attr(p, folded_scores=True))
    assert rc == -1 and E in msg and b"SAGE_ATTR_FP8_FOLDED_SCORES" in msg, msg
    rc, msg = _attn(lib, p, attr=_raw_attr(_cabi.ATTR_KV_SPLIT | (4 << 16) | _cabi.ATTR_FORCE_PERSISTENT, p, 1 << 30))
    assert rc == -1 and E in msg and b"SAGE_ATTR_FORCE_PERSISTENT" in msg, msg
    # the workspace: null, misaligned, short -- the size is _cabi.kv_split_ws_bytes of the shapes, named in the message
    for attr in (_raw_attr(_cabi.ATTR_KV_SPLIT | (4 << 16)), _attr(p + 64), _attr(p, nbytes=NEED - 1), _attr(p, nbytes=0)):
        rc, msg = _attn(lib, p, attr=attr)
        assert rc == -1 and E in msg and b"split workspace" in msg and f"{NEED} bytes".encode() in msg and b"128-byte aligned" in msg, (rc, msg)
    rc, msg = _attn(lib, p, attr=_attr(p, S=17, nbytes=0, gqa_pack=True), Hq=4, Lq=5)
    assert rc == -1 and f"{_cabi.kv_split_ws_bytes(1, 4, 5, 64, 17)} bytes".encode() in msg, msg
    # ... and with everything the split needs in place the next refusal is the one asked for, not the flag's
    for S in (2, 17, 255):
        rc, msg = _attn(lib, p, attr=_attr(p, S=S), D=96)
        assert rc == -1 and b"head_dim must be 64 or 128" in msg, (S, msg)
    for kw, match in ((dict(Lq=0), b"empty problem"), (dict(Hq=3, Hkv=2), b"divisible"), (dict(q=p + 2), b"16-byte aligned"), (dict(q_sl=68), b"q strides"),
                      (dict(k_sl=72), b"k strides"), (dict(o_sh=4), b"output strides"), (dict(q_dtype=2), b"q_dtype"), (dict(out_dtype=-1), b"out_dtype")):
        rc, msg = _attn(lib, p, **kw)
        assert rc == -1 and match in msg, (kw, rc, msg)
    rc, msg = _attn(lib, p, attr=_attr(p, gqa_pack=True), Hq=1)            # (what the entry takes of the attributes keeps the kv_lens entry's conditions)
    assert rc == -1 and b"SAGE_ATTR_GQA_PACK" in msg
    with pytest.raises(ValueError):
        _cabi.check(rc, "sage_kvpsplit_attn")
    # sage_kvpaged_attn refuses the flag as it did
    rc, msg = paged._attn(_cabi_kvpaged.load(), p, attr=_attr(p))
    assert rc == -1 and b"sage_kvpaged_attn: SAGE_ATTR_KV_SPLIT is not supported on a paged cache" in msg
    del buf


def test_two_violations_report_the_earlier_check():
    lib = _cabi_kvpsplit.load()
    buf, p = paged._aligned_buffer()
    checks = _order(p)
    for kw, match in checks:
        rc, msg = _attn(lib, p, **kw)
        assert rc == -1 and match in msg, (kw, rc, msg)
    covered = set()
    for (i, (kw_i, match_i)), (j, (kw_j, _)) in itertools.combinations(enumerate(checks), 2):
        if set(kw_i) & set(kw_j):                                    # two values for one argument do not fit into one call
            continue
        rc, msg = _attn(lib, p, **kw_i, **kw_j)
        assert rc == -1 and match_i in msg, (kw_i, kw_j, rc, msg)
        covered.add((i, j))
    # the checks of the attributes are on one argument: their order among themselves is pinned by pairs of flags in ONE struct
    split4 = _cabi.ATTR_KV_SPLIT | (4 << 16)
    for attr, kw, match in ((_raw_attr(_cabi.ATTR_KV_SPLIT | (1 << 16) | _cabi.ATTR_FP8_FOLDED_SCORES, p, 0, window=3), dict(Lq=200), b"2 .. 255"),
                            (_raw_attr(split4 | _cabi.ATTR_FP8_FOLDED_SCORES, p, 0, window=3), dict(Lq=200), b"Lq <= 128"),
                            (_raw_attr(split4 | _cabi.ATTR_FP8_FOLDED_SCORES, p, 0, window=3), dict(), b"no window"),
                            (_raw_attr(split4 | _cabi.ATTR_FP8_FOLDED_SCORES | _cabi.ATTR_FORCE_PERSISTENT, p, 0), dict(), b"SAGE_ATTR_FP8_FOLDED_SCORES"),
                            (_raw_attr(split4 | _cabi.ATTR_FORCE_PERSISTENT, p, 0), dict(), b"SAGE_ATTR_FORCE_PERSISTENT"),
                            (_raw_attr(4 << 16 | _cabi.ATTR_FP8_FOLDED_SCORES, p, 0, window=3), dict(Lq=200), b"attr must carry")):
        rc, msg = _attn(lib, p, attr=attr, **kw)
        assert rc == -1 and E in msg and match in msg, (kw, rc, msg)
    attr_rows = [i for i, (kw, _) in enumerate(checks) if "attr" in kw]
    assert all((i, i + 1) in covered for i in range(len(checks) - 1) if not (i in attr_rows and i + 1 in attr_rows)), sorted(covered)
    del buf


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
def _cache(dtype=torch.float16, seeded=True):
    c = PagedQuantizedKVCache.allocate(6, 128, 2, 2, 2, 64, dtype, "cpu")
    if seeded:
        c.seed(torch.zeros(2, 2, 64, dtype=dtype), torch.ones(2, 2, 64))
    return c


def test_value_errors_before_any_work():
    """The cache's own checks and the keywords' ValueErrors of the family's one resolver, in its order, on either kind of cache."""
    c = _cache()
    flat = QuantizedKVCache.allocate(2, 2, 256, 64, torch.float16, "cpu").seed(torch.zeros(2, 2, 64, dtype=torch.float16), torch.ones(2, 2, 64))
    q = torch.zeros(2, 4, 1, 64, dtype=torch.float16)
    for cache in (c, flat):
        for args, kw, match in (
                ((q.float(), cache, 4), {}, "dtype"),
                ((q.to("meta"), cache, 4), {}, "device"),
                ((torch.zeros(3, 4, 1, 64, dtype=torch.float16), cache, 4), {}, "B, D"),
                ((torch.zeros(2, 3, 1, 64, dtype=torch.float16), cache, 4), {}, "divisible"),
                ((q, "cache", 4), {}, "PagedQuantizedKVCache"),
                ((q, cache, 4), dict(tensor_layout="HDN"), "layout"),
                ((q, cache, 256), {}, "num_splits must be None, an int in"),
                ((q, cache, -1), {}, "num_splits must be None, an int in"),
                ((q, cache, True), {}, "num_splits must be None, an int in"),
                ((q, cache, 2.0), {}, "num_splits must be None, an int in"),
                ((q, cache, "most"), {}, "num_splits must be None, an int in"),
                ((torch.zeros(2, 4, 129, 64, dtype=torch.float16), cache, 4), {}, "num_splits needs qo_len <= 128"),
                ((torch.zeros(2, 4, 129, 64, dtype=torch.float16), cache, "auto"), dict(pack_gqa=1), "num_splits needs qo_len <= 128"),      # the earlier keyword's error
                ((q, cache, 4), dict(pack_gqa=1), "pack_gqa"),
                ((torch.zeros(2, 4, 33, 64, dtype=torch.float16), cache, 4), dict(pack_gqa=True), "qo_len <= 32"),
                ((torch.zeros(2, 2, 1, 64, dtype=torch.float16), cache, 4), dict(pack_gqa=True), "no GQA group"),
                ((q, cache, 4), dict(causal_align="middle"), "causal_align"),
                ((q, cache, 4), dict(causal_align="bottom_right"), "needs is_causal=True"),
                ((q, cache, 4), dict(q_start=1), "needs is_causal=True"),
                ((q, cache, 4), dict(is_causal=True, q_start=1, causal_align="bottom_right"), "not both"),
                ((q, cache, 4), dict(is_causal=True, q_start=torch.zeros(3, dtype=torch.int32)), r"shape \[B\]")):
            with pytest.raises(ValueError, match=match):
                sageattn_kvcache_split(*args, **kw)
    with pytest.raises(ValueError, match="no statistics"):
        sageattn_kvcache_split(q, _cache(seeded=False), 4)
    with pytest.raises(TypeError):                                    # window_size is not offered
        sageattn_kvcache_split(q, c, 4, window_size=(70, 0))
    with pytest.raises(TypeError):                                    # num_splits is the call's point: positional, required
        sageattn_kvcache_split(q, c)


def test_sageattn_kvcache_still_refuses_num_splits_on_a_paged_cache():
    c = _cache()
    q = torch.zeros(2, 4, 1, 64, dtype=torch.float16)
    for ns in (2, "auto", 1, 0):
        with pytest.raises(ValueError, match="num_splits is not supported on a PagedQuantizedKVCache"):
            sageattn_kvcache(q, c, num_splits=ns)
    import inspect
    par = inspect.signature(sageattn_kvcache_split).parameters
    assert list(par) == ["q", "cache", "num_splits", "tensor_layout", "is_causal", "causal_align", "q_start", "pack_gqa", "sm_scale", "return_lse"]
    assert [par[n].default for n in list(par)[3:]] == ["HND", False, "top_left", None, False, None, False]
    assert list(inspect.signature(sageattn_kvcache).parameters) == ["q", "cache", "tensor_layout", "is_causal", "causal_align", "q_start", "window_size",
                                                                   "pack_gqa", "num_splits", "sm_scale", "return_lse"]


# ---- the build --------------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include "sage_attn_form.h"
#include <cstdio>
using namespace sage;
int main()
{
    for (int D : {128, 64}) {
        const FormList l = unit_forms(UNIT_F8KS, D);
        for (int i = 0; i < l.n; i++) printf("%d %u %d\n", D, l.v[i], min_waves(unpack(l.v[i])));
    }
    return 0;
}
"""
UNITS = ["sage_attn_d128_f8pks.hip", "sage_attn_d64_f8pks.hip"]


@pytest.fixture(scope="module")
def listed(tmp_path_factory):
    """{D: {packed form: min_waves}} of unit_forms(UNIT_F8KS, D), read from the header with a small host program"""
    tmp = tmp_path_factory.mktemp("paged_split_forms")
    src, exe = tmp / "forms.hip", tmp / "forms"
    src.write_text(PROGRAM)
    out = subprocess.run([tbr.HIPCC, "-std=c++17", "--cuda-host-only", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lists = {}
    for line in run.stdout.strip().split("\n"):
        D, word, waves = line.split()
        lists.setdefault(int(D), {})[int(word)] = int(waves)
    return lists


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_new_units_hold_the_paged_kernels_of_the_split_without_scratch(listed):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert all(s in srcs for s in UNITS + ["sage_split_paged.hip", "sage_split_exact.hip"])
    assert "sage_kvpsplit_gfx950.h" in re.search(r"^HDRS\s*:=\s*(.*)$", mk, re.M).group(1)
    todo = UNITS + ["sage_split_paged.hip"]
    with ThreadPoolExecutor(max_workers=len(todo)) as ex:
        reports = dict(zip(todo, ex.map(tbr._resource_report, todo)))
    for unit in UNITS:
        D = 128 if "d128" in unit else 64
        rep, want = reports[unit], listed[D]
        assert len(want) == 8
        assert not [k for k in rep if "sage_attn_kernel" in k], "an unpaged kernel in a paged unit"
        mine = {k: v for k, v in rep.items() if "sage_attn_paged_kernel" in k}
        assert {kf.pack(kf.decode_paged(k)) for k in mine} == set(want) and len(mine) == 8, (unit, sorted(mine))
        for name, res in mine.items():
            f = kf.decode_paged(name)
            assert f["D"] == D and f["kvlen"] and f["seed"] and not f["window"] and f["qstart"] == f["causal"] and kf.encode_paged(f) == name
            assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0 and res["ScratchSize"] == 0, (name, res)
            assert res["Occupancy"] >= want[kf.pack(f)] == (2 if D == 128 else 3), (name, res)
        assert {(f["causal"], f["gpack"], f["qf"]) for f in map(kf.decode_paged, mine)} == set(itertools.product((False, True), (False, True), (1, 2)))
    p1 = {k: v for k, v in reports["sage_split_paged.hip"].items() if "chunk_max_lens_paged_kernel" in k}
    assert len(p1) == 8 and len(reports["sage_split_paged.hip"]) == 8, sorted(reports["sage_split_paged.hip"])
    for name, res in p1.items():
        assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0 and res["ScratchSize"] == 0 and res["Occupancy"] >= 2, (name, res)


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_lint_walks_the_new_units_without_a_finding():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_hazard_lint as lint
    assert lint.UNITS_PAGED_SPLIT == tuple(UNITS)
    assert lint.UNITS_PAGED == ("sage_attn_d128_f8p.hip", "sage_attn_d64_f8p.hip", "sage_attn_d128_f8pg.hip", "sage_attn_d64_f8pg.hip")
    assert lint.UNITS_KV_SPLIT == ("sage_attn_d128_f8ks.hip", "sage_attn_d64_f8ks.hip")
    with ThreadPoolExecutor(max_workers=2) as ex:
        results = dict(zip(UNITS, ex.map(lambda u: lint.lint(lint.listing(u)), UNITS)))
    for unit, (findings, n_mfma) in results.items():
        assert n_mfma >= 200, (unit, n_mfma)                   # (the walk did see the pipelined loops)
        assert not findings, (unit, findings[:5])


# ---- which table entries a paged split call may read -----------------------------------------------------------------------------------
def may_read(causal, Lq, page_size, max_pages, len_b, s_b, S):
    """bool [max_pages]: the table entries of sample b that a paged split call of S chunks may read (pass 2, whose tiles contain pass 1's).
    Chunk c runs on keys [kc0, kc0 + lk) of the logical axis (``loop_plan.split_chunk``); a chunk without keys (lk = 0) or wholly behind the
    diagonal of the work item's 128-row query block (n_iters = 0: the kernel's bound is the block's, whatever Lq) requests no tile; any other
    chunk looks up tiles kc0 / 64 .. kc0 / 64 + ceil(lk / 64) - 1 and no others -- where the body looks ahead it clamps to that last tile."""
    cap = page_size * max_pages
    shift = (page_size // 64).bit_length() - 1
    out = np.zeros(max_pages, dtype=bool)
    for c in range(S):
        p = lp.split_chunk(causal, Lq, cap, len_b, s_b if causal else None, S, c)
        if p.lk == 0 or p.n_iters == 0:
            continue
        t0 = p.kc0 // 64
        tiles = np.arange(t0, t0 + (p.lk + 63) // 64)
        out[tiles >> shift] = True
    return out


def _pages(*idx, n):
    out = np.zeros(n, dtype=bool)
    out[list(idx)] = True
    return out


HAND = [
    # (causal, Lq, page_size, max_pages, len, s, S) -> the entries, written out by hand
    # pages of 128 keys, capacity 1152 = 18 tiles, S 4: T = 5.  700 keys are 11 tiles: chunks 0 / 1 / 2 hold tiles 0-4 / 5-9 / 10, chunk 3 none
    ((False, 1, 128, 9, 700, None, 4), (0, 1, 2, 3, 4, 5)),
    ((False, 1, 128, 9, 0, None, 4), ()),                                   # a sample without keys reads none
    ((False, 1, 128, 9, 1, None, 4), (0,)),
    ((False, 33, 128, 9, 5000, None, 17), tuple(range(9))),                 # the length is clamped to the capacity
    ((False, 1, 128, 9, -3, None, 2), ()),
    # causal, five rows at offset 100: the block's last row (127) sees key 227.  Chunk 0 holds tiles 0-4 and runs (its tiles behind the diagonal
    # are not iterated, but the body's look-ahead may name any tile of the chunk); chunk 1 starts at key 320, behind the block: no lookup at all
    ((True, 5, 128, 9, 700, 100, 4), (0, 1, 2)),
    ((True, 5, 128, 9, 700, 320, 4), (0, 1, 2, 3, 4)),                      # row 0 sees key 320, the first of chunk 1 (tiles 5-9: pages 2-4)
    ((True, 5, 128, 9, 700, -5, 4), (0, 1, 2)),                             # every row that exists in front of key 0: chunk 0 still runs (the block's bound)
    ((True, 5, 128, 9, 700, 695, 4), (0, 1, 2, 3, 4, 5)),                   # bottom-right
    # pages of 64 keys, capacity 1088 = 17 tiles, S 17: T = 1, a chunk is a page
    ((False, 1, 64, 17, 321, None, 17), (0, 1, 2, 3, 4, 5)),
    ((True, 1, 64, 17, 321, 130, 17), (0, 1, 2, 3, 4)),                     # the block's last row sees key 257: chunks 0 .. 4 (key 256) run
    # pages of 256 keys, capacity 2560 = 40 tiles, S 3: T = 14; chunk 1 starts at tile 14 = tile 2 of page 3, chunk 2 at tile 28 = page 7
    ((False, 16, 256, 10, 897, None, 3), (0, 1, 2, 3)),                     # 15 tiles: chunk 1 holds tile 14 alone
    ((False, 16, 256, 10, 896, None, 3), (0, 1, 2, 3)),                     # 14 tiles: chunk 0 alone, whose last tile is tile 1 of page 3
    ((False, 16, 256, 10, 2560, None, 3), tuple(range(10))),
    # the last row sees key 1815, in tile 28 -- chunk 2's first tile -- so chunk 2 RUNS and may look up every tile it holds (28 .. 39: pages 7 .. 9):
    # "may read" is per chunk, not per visible key
    ((True, 16, 256, 10, 2560, 1800, 3), tuple(range(10))),
    ((True, 16, 256, 10, 2560, 1600, 3), tuple(range(7))),                  # the block's last row sees key 1727 < 1792: chunk 2 does not run
]


def test_the_restatement_gives_the_hand_written_entries():
    for i, (args, pages) in enumerate(HAND):
        got = may_read(*args)
        assert np.array_equal(got, _pages(*pages, n=args[3])), (i, args, np.flatnonzero(got).tolist(), pages)


def test_no_entry_behind_the_length_and_none_of_a_chunk_that_does_not_run():
    """Over a sweep: every entry that may be read lies in front of ceil(len / page_size); non-causal it is exactly those; causal, the entries are
    those of the chunks that hold a key the work item's 128-row block sees."""
    for page_size, max_pages in ((64, 17), (128, 9), (256, 10)):
        cap = page_size * max_pages
        for S in (2, 3, 4, 17, 255):
            T = lp.split_tiles(cap, S)
            for n in (0, 1, 63, 64, 65, 320, 321, 700, cap - 1, cap, cap + 5):
                lenb = max(0, min(n, cap))
                need = -(-lenb // page_size)
                got = may_read(False, 16, page_size, max_pages, n, None, S)
                assert np.array_equal(got, np.arange(max_pages) < need), (page_size, S, n)
                for s in (-20, -16, 0, 37, 64, 300, lenb - 16, cap):
                    got = may_read(True, 16, page_size, max_pages, n, s, S)
                    assert not got[need:].any(), (page_size, S, n, s)
                    sc = max(-16, min(s, cap))
                    last_visible = min(lenb - 1, sc + 127)                 # the last key the 128-row block sees (negative: none)
                    want = np.zeros(max_pages, dtype=bool)
                    for c in range(S):
                        k0, k1 = c * 64 * T, min((c + 1) * 64 * T, lenb)
                        if k0 < k1 and k0 <= last_visible:
                            want[k0 // page_size:-(-k1 // page_size)] = True
                    assert np.array_equal(got, want), (page_size, S, n, s, np.flatnonzero(got).tolist(), np.flatnonzero(want).tolist())


def test_the_gpu_tests_selection_covers_its_kinds():
    """tests/test_gpu_paged_split.py chooses its lengths and offsets with the same model; what they cover is asserted here too, without a GPU."""
    import test_gpu_paged_split as g
    g.test_the_shapes_are_what_the_docstring_says()
    g.test_the_loop_selection_covers_what_it_is_for()
