"""CPU: the page pool of the paged KV cache -- C boundary, Python interface, the pool arithmetic, the build (include/sage_kvpool_gfx950.h,
sageattention_amd/_cabi_kvpool.py, sageattention_amd/paged_kv_pool.py, csrc/sage_page_pool.h, csrc/sage_kv_pool.hip).  The host twins run the
header's functions and are held word for word to a model written from the statement of the arithmetic (tests/ref_page_pool.py) over seeded
random serving programs that must reach every corner; the invariants hold after every operation; the arithmetic keeps every index inside its
array over hostile words (a stand-alone program under AddressSanitizer and UBSan); the header's prototypes are the binding's table; every
argument error returns -1 in the header's order; the Python layer raises ValueError before any work; the new unit builds without scratch --
and none of it moved what the other headers, bindings and units pin."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import util  # noqa: F401  (sys.path)
import ref_page_pool as rpp
import test_build_resources as tbr
import test_paged_kv_host as paged
from test_kv_cache_host import MAIN_HEADER, _prototypes, _text

ROOT = tbr.ROOT
CSRC = os.path.join(ROOT, "sageattention_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "sage_kvpool_gfx950.h")
ENTRIES = sorted(["sage_kvpool_abi_version", "sage_kvpool_ws_bytes"] +
                 [f"sage_kvpool_{op}{twin}" for op in ("init", "reserve", "release", "fork_prepare") for twin in ("", "_host")])
N_PROGRAMS = 240
CORNERS = {"dry", "refused_in_the_middle", "block_edge", "page_edge", "capacity_edge", "fork_page_edge", "fork_full_table", "several_forks_of_one_source",
           "two_released_share", "one_sharer_released_first", "fork_dry"}


def _pool_binding():
    from sageattention_amd import _cabi_kvpool
    return _cabi_kvpool


# ---- the boundary -------------------------------------------------------------------------------------------------------------------------------
def test_binding_is_the_header():
    kvpool = _pool_binding()
    protos = _prototypes(HEADER, "SAGE_KVPOOL_API")
    assert sorted(protos) == sorted(kvpool.SYMBOLS) == ENTRIES
    for name, (ret, params) in protos.items():
        res, argtypes = kvpool.SYMBOLS[name]
        assert res is paged._ctype(ret), f"{name}: returns {ret}, bound as {res}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters declared, {len(argtypes)} bound"
        for i, (ctype, bound) in enumerate(zip(params, argtypes)):
            assert bound is paged._ctype(ctype), f"{name}: parameter {i} ({ctype}) bound as {bound}"
    version = int(re.search(r"#define\s+SAGE_KVPOOL_ABI_VERSION\s+(\d+)", _text(HEADER)).group(1))
    assert version == 1 == kvpool.ABI_VERSION
    rest = re.sub(r"SAGE_KVPOOL_API", "", _text(HEADER))
    assert "SAGE_API" not in rest and "SAGE_KVFORK_API" not in rest and "SAGE_KVPAGED_API" not in rest            # an export macro of its own
    assert "sage_kvpool_gfx950.h" in open(os.path.join(CSRC, "Makefile")).read()
    # a device entry and its host twin differ in the trailing stream alone
    for op in ("init", "reserve", "release", "fork_prepare"):
        dev, host = protos[f"sage_kvpool_{op}"], protos[f"sage_kvpool_{op}_host"]
        assert dev[0] == host[0] and dev[1][:-1] == host[1] and dev[1][-1] == "void *", op


def test_library_exports_the_entries_and_the_other_boundaries_did_not_move():
    from sageattention_amd import _cabi, _cabi_kvcache, _cabi_kvfork, _cabi_kvlist, _cabi_kvpaged, _cabi_kvpsplit, _cabi_kvpvarlen, _cabi_kvstep
    import sageattention_amd as sa
    kvpool = _pool_binding()
    lib = ctypes.CDLL(_cabi.LIB_PATH)
    for name in kvpool.SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
    assert kvpool.load() is _cabi.load() and kvpool.load().sage_kvpool_abi_version() == 1
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22
    assert len(_prototypes(MAIN_HEADER, "SAGE_API")) == 56 and len(_cabi.SYMBOLS) == 56
    seven = ((_cabi_kvcache, "kvcache", 2), (_cabi_kvpaged, "kvpaged", 3), (_cabi_kvfork, "kvfork", 2), (_cabi_kvpsplit, "kvpsplit", 2),
             (_cabi_kvpvarlen, "kvpvarlen", 3), (_cabi_kvstep, "kvstep", 2), (_cabi_kvlist, "kvlist", 5))
    for binding, stem, count in seven:
        header = os.path.join(ROOT, "include", f"sage_{stem}_gfx950.h")
        protos = _prototypes(header, f"SAGE_{stem.upper()}_API")
        assert sorted(protos) == sorted(binding.SYMBOLS) and len(protos) == count, stem
        assert getattr(binding.load(), f"sage_{stem}_abi_version")() == binding.ABI_VERSION == 1, stem
        assert int(re.search(rf"#define\s+SAGE_{stem.upper()}_ABI_VERSION\s+(\d+)", _text(header)).group(1)) == 1, stem
        assert not any(n.startswith("sage_kvpool") for n in binding.SYMBOLS)
        assert not any(n.startswith(f"sage_{stem}") for n in kvpool.SYMBOLS)
    assert not any(n.startswith("sage_kvpool") for n in _cabi.SYMBOLS)
    assert "PagePool" not in sa.__all__ and "paged_kv_pool" not in sa.__all__ and not hasattr(sa, "PagePool")


def _np(x):
    return None if x is None else x.ctypes.data


def _geom(p, **kw):
    a = dict(ws=p, ws_bytes=4096, table=p, bt_stride=2, num_pages=4, page_size=64, mp=2, B=1)
    a.update(kw)
    return a


def _call(lib, entry, a, stream):
    rc = getattr(lib, entry)(*a.values(), *stream)
    return rc, lib.sage_last_error()


def test_every_argument_error_returns_minus_one_in_the_headers_order():
    lib = _pool_binding().load()
    buf, p = paged._aligned_buffer()
    geometry = [(dict(table=None), b"null block_table"), (dict(page_size=96), b"page_size must be 64 * 2^k"), (dict(num_pages=0), b"num_pages must be at least 1"),
                (dict(mp=0), b"max_pages_per_seq must be at least 1")]
    ws_small = (dict(ws_bytes=4 * (16 + 8 + 1) - 1), b"pool_ws holds 99 bytes, sage_kvpool_ws_bytes(num_pages, B) = 100")
    b_range = (dict(B=1025), b"B must be in 1 .. 1024")
    n_range = (dict(n=1025), b"n must be in 1 .. 1024")
    cases = {
        "reserve": (dict(lens=p, new_lens=p, T=1, cu=None, total=1, max_new=1, granted=p),
                    geometry + [(dict(lens=None), b"null pool_ws, lens or granted"), (dict(cu=p), b"pass exactly one of new_lens"),
                                (dict(granted=p + 2), b"must be 4-byte aligned"), b_range, (dict(T=0), b"T must be at least 1"), ws_small]),
        "release": (dict(lens=p, slots=p, n=1),
                    geometry + [(dict(slots=None), b"null pool_ws, lens or slots"), (dict(lens=p + 1), b"must be 4-byte aligned"), b_range, n_range, ws_small]),
        "fork_prepare": (dict(lens=p, src=p, dst=p, prefix=None, n=1, new_pages=p, dst_eff=p),
                         geometry + [(dict(dst_eff=None), b"null pool_ws, lens, src_slots, dst_slots, new_pages or dst_eff"),
                                     (dict(prefix=p + 2), b"must be 4-byte aligned"), b_range, n_range, ws_small]),
    }
    for op, (extra, checks) in cases.items():
        for entry, stream in ((f"sage_kvpool_{op}", (None,)), (f"sage_kvpool_{op}_host", ())):
            e = entry.encode() + b": "
            base = dict(_geom(p), **extra)                               # (an update of a key keeps its place: the values stay in the entry's order)
            for kw, match in checks:                                     # each violation alone gives its own message, under the entry's own name
                rc, msg = _call(lib, entry, dict(base, **kw), stream)
                assert rc == -1 and msg.startswith(e) and match in msg, (entry, kw, rc, msg)
            for (kw_i, match_i), (kw_j, _) in itertools.combinations(checks, 2):       # of two violations the earlier check speaks
                if set(kw_i) & set(kw_j):
                    continue
                rc, msg = _call(lib, entry, dict(base, **kw_i, **kw_j), stream)
                assert rc == -1 and match_i in msg, (entry, kw_i, kw_j, rc, msg)
    # reserve: neither array, and the packed form's host numbers
    a = dict(_geom(p), lens=p, new_lens=None, T=1, cu=None, total=1, max_new=1, granted=p)
    assert _call(lib, "sage_kvpool_reserve", a, (None,))[0] == -1 and b"pass exactly one of" in lib.sage_last_error()
    a.update(cu=p, max_new=0)
    assert _call(lib, "sage_kvpool_reserve_host", a, ())[0] == -1 and b"total and max_new must be at least 1" in lib.sage_last_error()
    # init and the workspace's size
    for entry, stream in (("sage_kvpool_init", (None,)), ("sage_kvpool_init_host", ())):
        for kw, match in ((dict(num_pages=0), b"num_pages must be at least 1"), (dict(ws=None), b"null pool_ws"), (dict(ws=p + 2), b"4-byte aligned"),
                          (dict(B=0), b"B must be in 1 .. 1024"), (dict(ws_bytes=4 * 25 - 1), b"pool_ws holds 99 bytes")):
            a = dict(dict(ws=p, ws_bytes=4096, num_pages=4, B=1), **kw)
            rc, msg = _call(lib, entry, a, stream)
            assert rc == -1 and msg.startswith(entry.encode() + b": ") and match in msg, (entry, kw, msg)
    assert lib.sage_kvpool_ws_bytes(4, 1) == 100 and lib.sage_kvpool_ws_bytes(54, 6) == 4 * (16 + 108 + 6) and lib.sage_kvpool_ws_bytes(1 << 30, 1024) == 4 * (16 + (1 << 31) + 1024)
    for bad in ((0, 1), (1, 0)):
        assert lib.sage_kvpool_ws_bytes(*bad) == -1 and b"sage_kvpool_ws_bytes" in lib.sage_last_error()
    from sageattention_amd import _cabi
    with pytest.raises(ValueError):
        _cabi.check(-1, "sage_kvpool_reserve")
    del buf


# ---- the host twins against the model -----------------------------------------------------------------------------------------------------------
class HostPool:
    """The *_host entries over numpy arrays, shaped like ref_page_pool.PoolModel."""

    def __init__(self, N, B, ps, mp):
        self.lib = _pool_binding().load()
        self.N, self.B, self.ps, self.mp, self.cap = N, B, ps, mp, mp * ps
        self.ws = np.full(rpp.HDR + 2 * N + B, 0x5A5A5A5A, dtype=np.int32)
        self.table = np.full((B, mp), -1, dtype=np.int32)
        self.lens = np.zeros(B, dtype=np.int32)
        self.init()

    def _geom(self):
        return (_np(self.ws), self.ws.nbytes, _np(self.table), self.mp, self.N, self.ps, self.mp, self.B)

    def _ok(self, rc):
        assert rc == 0, self.lib.sage_last_error()

    def init(self):
        self._ok(self.lib.sage_kvpool_init_host(_np(self.ws), self.ws.nbytes, self.N, self.B))

    def reserve(self, new_lens=None, T=1, cu=None, total=1, max_new=1):
        granted = np.full(self.B, -7, dtype=np.int32)
        self._ok(self.lib.sage_kvpool_reserve_host(*self._geom(), _np(self.lens), _np(new_lens), T, _np(cu), total, max_new, _np(granted)))
        return granted

    def release(self, slots):
        slots = np.asarray(slots, dtype=np.int32)
        self._ok(self.lib.sage_kvpool_release_host(*self._geom(), _np(self.lens), _np(slots), len(slots)))

    def fork_prepare(self, src, dst, prefix_lens=None):
        pages, eff = np.full(len(src), -7, dtype=np.int32), np.full(len(src), -7, dtype=np.int32)
        self._ok(self.lib.sage_kvpool_fork_prepare_host(*self._geom(), _np(self.lens), _np(src), _np(dst), _np(prefix_lens), len(src), _np(pages), _np(eff)))
        return pages, eff


def run_host_op(h, m, op):
    """One op on the host twins, with the table and the lengths moved as the model's helpers move them (no cache here)."""
    if op[0] == "reserve_dense":
        return h.reserve(new_lens=op[1], T=op[2]), None, None
    if op[0] == "reserve_packed":
        return h.reserve(cu=op[1], total=op[2], max_new=op[3]), None, None
    if op[0] == "release":
        h.release(op[1])
        return None, None, None
    if op[0] == "fork":
        pages, eff = h.fork_prepare(op[1], op[2], op[3])
        return None, pages, eff
    h.init()
    h.table[:] = -1
    h.lens[:] = 0
    return None, None, None


def test_host_twins_equal_the_model_word_for_word_on_random_programs():
    reached, n_ops = {}, 0
    for seed in range(N_PROGRAMS):
        N, B, ps, mp, ops, corners = rpp.random_program(seed)
        for c in corners:
            reached[c] = reached.get(c, 0) + 1
        m, h = rpp.PoolModel(N, B, ps, mp), HostPool(N, B, ps, mp)
        assert (h.ws == m.ws).all(), seed
        # the append and sage_kvfork are not part of this test: what they do to the lengths and the table is done by the model's two helpers, on
        # the host twins' own arrays and from the host twins' own answers
        after = rpp.PoolModel(N, B, ps, mp)
        after.table, after.lens = h.table, h.lens
        for k, op in enumerate(ops):
            want = rpp.run_op(m, op)
            got = run_host_op(h, m, op)
            if got[0] is not None:
                after.advance(got[0])
            if op[0] == "fork":
                after.apply_fork(op[1], got[2], got[1], op[3])
            for name, a, b in zip(("granted", "new_pages", "dst_eff"), got, want):
                assert (a is None and b is None) or (a == b).all(), (seed, k, op[0], name, a, b)
            assert (h.ws == m.ws).all(), (seed, k, op[0], h.ws[:16], m.ws[:16])
            assert (h.table == m.table).all() and (h.lens == m.lens).all(), (seed, k, op[0])
            m.check_invariants()
            n_ops += 1
        m.release(list(range(B)))
        h.release(list(range(B)))
        assert (h.ws == m.ws).all() and m.hdr[0] == N and (m.table == -1).all() and sorted(m.stack.tolist()) == list(range(N)), seed
    assert set(reached) == CORNERS and min(reached.values()) >= 3, reached
    assert n_ops >= 10 * N_PROGRAMS


def test_hand_checked_steps():
    # 5 pages of 64 keys, 3 slots, up to 4 pages each.  Page 0 first.
    h = HostPool(5, 3, 64, 4)
    assert h.ws[:16].tolist() == [5] + [0] * 15 and h.ws[16:21].tolist() == [4, 3, 2, 1, 0]
    g = h.reserve(new_lens=np.array([65, 0, 64], dtype=np.int32), T=65)          # slot 0: two pages (0, 1), slot 2: one (2)
    assert g.tolist() == [65, 0, 64] and h.table.tolist() == [[0, 1, -1, -1], [-1] * 4, [2, -1, -1, -1]] and h.ws[:4].tolist() == [2, 0, 0, 0]
    h.lens[:] = [65, 0, 64]
    # slot 0 fits its row into page 1; slot 1 asks for three of two free pages and is refused; slot 2 behind it asks for one and is refused as well
    # (the refused need counts); two refusals, 4 - 2 = 2 pages short
    g = h.reserve(new_lens=np.array([1, 129, 1], dtype=np.int32), T=129)
    assert g.tolist() == [1, 0, 0] and h.ws[:4].tolist() == [2, 2, 2, 2] and h.table[1].tolist() == [-1] * 4
    h.lens[0] = 66
    # fork 0 -> 1 on the block boundary 64: one shared page, a page of its own (3); the count of page 0 is 2
    pages, eff = h.fork_prepare(np.array([0, 0], dtype=np.int32), np.array([1, 2], dtype=np.int32), np.array([64, 64], dtype=np.int32))
    assert pages.tolist() == [3, -1] and eff.tolist() == [1, -1] and h.ws[:4].tolist() == [1, 1, 0, 3]           # slot 2 is not empty
    assert h.ws[16 + 5:16 + 10].tolist() == [2, 1, 1, 1, 0] and h.ws[16 + 10:].tolist() == [2, 2, 1]
    h.table[1, :2] = [0, 3]
    h.lens[1] = 64
    # releasing the parent frees page 1 alone; then the child and slot 2: pages 3, 2, 0 pushed so that 0 comes first
    h.release([0])
    assert h.ws[:1].tolist() == [2] and h.ws[16:18].tolist() == [4, 1] and h.ws[16 + 5:16 + 10].tolist() == [1, 0, 1, 1, 0] and h.lens.tolist() == [0, 64, 64]
    h.release([2, 1, 7])
    assert h.ws[0] == 5 and h.ws[16:21].tolist() == [4, 1, 3, 2, 0] and (h.ws[21:] == 0).all() and (h.table == -1).all() and (h.lens == 0).all()


# ---- the arithmetic over hostile words ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_pool_holds_over_hostile_words_under_the_sanitizers(tmp_path):
    """tests/page_pool_main.cpp: a program of its own (no GPU, nothing loaded into this process), AddressSanitizer and UBSan on the host."""
    exe = tmp_path / "page_pool"
    host = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    out = subprocess.run([tbr.HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", *host, "-I", CSRC,
                          os.path.join(ROOT, "tests", "page_pool_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    syms = subprocess.run(["nm", str(exe)], capture_output=True, text=True, timeout=60).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the program was built without the sanitizers"
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=240)
    assert run.returncode == 0 and "every index inside, every id a page" in run.stdout and "runtime error" not in run.stderr and \
        "AddressSanitizer" not in run.stderr, (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    # one definition: the header includes the ragged clamp alone and states none of its own; the unit reads the header
    text = open(os.path.join(CSRC, "sage_page_pool.h")).read()
    assert re.findall(r"#include\s+(\S+)", text) == ['"sage_ragged.h"'] and text.count("ragged_rows(") == 1 and "q1 - q0" not in text
    assert '#include "sage_page_pool.h"' in open(os.path.join(CSRC, "sage_kv_pool.hip")).read()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------------
def test_value_errors_before_any_work():
    from sageattention_amd.kv_cache import QuantizedKVCache
    from sageattention_amd.paged_kv_pool import PagePool
    with pytest.raises(ValueError, match="PagePool takes a PagedQuantizedKVCache"):
        PagePool(QuantizedKVCache.allocate(2, 2, 64, 64, torch.float16, "cpu"))
    with pytest.raises(ValueError, match="PagePool takes a PagedQuantizedKVCache"):
        PagePool("cache")
    big = paged.PagedQuantizedKVCache.allocate(6, 128, 1025, 2, 2, 64, torch.float16, "meta")
    with pytest.raises(ValueError, match="at most 1024 sequence slots"):
        PagePool(big)
    c = paged._cache(seeded=True)                # B 2, Hkv 2, D 64, fp16, 6 pages of 128, two per sequence, on the CPU
    pool = PagePool(c, _init=False)
    assert pool.ws.shape == (16 + 12 + 2,) and pool.ws.dtype == torch.int32
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32)
    k = torch.zeros(2, 2, 3, 64, dtype=torch.float16)
    for call, match in (
            (lambda: pool.reserve(), "exactly one of"),
            (lambda: pool.reserve(new_lens=i32(1, 1), T=1, cu_seqlens=i32(0, 1, 2), max_new=1), "exactly one of"),
            (lambda: pool.reserve(new_lens=i32(1, 1)), "T must be a positive int"),
            (lambda: pool.reserve(new_lens=i32(1, 1), T=True), "T must be a positive int"),
            (lambda: pool.reserve(new_lens=i32(1, 1, 1), T=1), r"shape \[B\]"),
            (lambda: pool.reserve(new_lens=torch.zeros(2), T=1), "new_lens must be an int32 or int64 tensor"),
            (lambda: pool.reserve(cu_seqlens=i32(0, 1), max_new=1, total=1), r"shape \[B \+ 1\]"),
            (lambda: pool.reserve(cu_seqlens=i32(0, 1, 2), max_new=0, total=2), "max_new must be a positive int"),
            (lambda: pool.reserve(cu_seqlens=i32(0, 1, 2), max_new=1), "total must be a positive int"),
            (lambda: pool.release([]), "at least one slot"),
            (lambda: pool.release([0, 0]), "distinct"),
            (lambda: pool.release([2]), "distinct indices in"),
            (lambda: pool.release(torch.zeros(2)), "slots must be"),
            (lambda: pool.fork([0], [1, 0]), "one length"),
            (lambda: pool.fork([0], [2]), "dst_slots must be slot indices"),
            (lambda: pool.fork([0, 0], [1, 1]), "dst_slots must be distinct"),
            (lambda: pool.fork([0], [0]), "disjoint"),
            (lambda: pool.fork([], []), "one length"),
            (lambda: pool.append(k, k, new_lens=torch.zeros(2)), "new_lens must be an int32 or int64 tensor"),
            (lambda: pool.append(k[0], k), "4-D")):
        with pytest.raises(ValueError, match=match):
            call()
    unseeded = PagePool(paged._cache(seeded=False), _init=False)
    with pytest.raises(ValueError, match="no statistics"):
        unseeded.fork([0], [1])
    # the cache class and its module are what they were but for a pointer in the docstring
    text = open(os.path.join(ROOT, "sageattention_amd", "paged_kv_cache.py")).read()
    assert "import" in text and "_cabi_kvpool" not in text and "from .paged_kv_pool" not in text


# ---- the build ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_pool_unit_is_built_and_uses_no_scratch():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "sage_kv_pool.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    rep = tbr._resource_report("sage_kv_pool.hip")
    assert sorted(rep) == ["_ZN4sage19kv_pool_init_kernelEPiii", "_ZN4sage22kv_pool_release_kernelENS_12KvPoolParamsE", "_ZN4sage22kv_pool_reserve_kernelENS_12KvPoolParamsE",
                           "_ZN4sage27kv_pool_fork_prepare_kernelENS_12KvPoolParamsE"], sorted(rep)
    for name, res in rep.items():
        assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0 and res.get("SGPRs Spill", 0) == 0, (name, res)
        assert res["VGPRs"] <= 64, (name, res)           # one workgroup of 1024 threads: 16 waves on a CU need no more than 128; these are small kernels
