"""CPU: the fork of paged KV-cache sequences -- its C boundary, Python interface, build and numpy restatement (include/sage_kvfork_gfx950.h,
sageattention_amd/_cabi_kvfork.py, ``PagedQuantizedKVCache.fork``, csrc/sage_kv_fork.hip, tests/ref_kvfork.py).  The header's prototypes are
the binding's table, the library exports them, every argument error returns -1 with its message before anything touches a GPU and in the
order the header lists, the Python layer raises ValueError before any work, the unit holds one kernel per head size without scratch -- and
``ref_kvfork.fork_state``, from which the GPU tests take their expectations, gives what the header says on cases written out by hand."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import util  # noqa: F401  (sys.path)
import ref_kvfork
import test_build_resources as tbr
from sageattention_amd import _cabi, _cabi_kvcache, _cabi_kvfork, _cabi_kvpaged
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
from test_kv_cache_host import _ctype_of, _prototypes, _text
from test_paged_kv_host import BAD_PAGE_SIZES, _aligned_buffer

ROOT = tbr.ROOT
HEADER = os.path.join(ROOT, "include", "sage_kvfork_gfx950.h")
ENTRIES = ["sage_kvfork", "sage_kvfork_abi_version"]


def _ctype(ctype):
    return ctypes.c_void_p if ctype.endswith("*") else _ctype_of(ctype)


def test_binding_is_the_header():
    protos = _prototypes(HEADER, "SAGE_KVFORK_API")
    assert sorted(protos) == sorted(_cabi_kvfork.SYMBOLS) == ENTRIES
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_kvfork.SYMBOLS[name]
        assert res is _ctype(ret), f"{name}: returns {ret}, bound as {res}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters declared, {len(argtypes)} bound"
        for i, (ctype, bound) in enumerate(zip(params, argtypes)):
            assert bound is _ctype(ctype), f"{name}: parameter {i} ({ctype}) bound as {bound}"
    version = int(re.search(r"#define\s+SAGE_KVFORK_ABI_VERSION\s+(\d+)", _text(HEADER)).group(1))
    assert version == 1 == _cabi_kvfork.ABI_VERSION
    rest = re.sub(r"SAGE_KVFORK_API", "", _text(HEADER))
    assert "SAGE_API" not in rest and "SAGE_KVCACHE_API" not in rest and "SAGE_KVPAGED_API" not in rest          # an export macro of its own
    assert "rounded down" in open(HEADER).read().lower()                                                        # the prefix rounding is documented


def test_library_exports_the_entries():
    lib = ctypes.CDLL(_cabi.LIB_PATH)
    for name in _cabi_kvfork.SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
    assert _cabi_kvfork.load() is _cabi.load()                       # one library, bound behind _cabi.load()
    assert _cabi_kvfork.load().sage_kvfork_abi_version() == 1


def test_the_older_symbol_tables_hold_no_fork_name():
    older = list(_cabi.SYMBOLS) + list(_cabi_kvcache.SYMBOLS) + list(_cabi_kvpaged.SYMBOLS)
    assert not any(n.startswith("sage_kvfork") for n in older)
    assert (_cabi.ABI_VERSION, _cabi_kvcache.ABI_VERSION, _cabi_kvpaged.ABI_VERSION) == (22, 1, 1)
    for h, macro in (("sage_gfx950.h", "SAGE_API"), ("sage_kvcache_gfx950.h", "SAGE_KVCACHE_API"), ("sage_kvpaged_gfx950.h", "SAGE_KVPAGED_API")):
        assert not any(n.startswith("sage_kvfork") for n in _prototypes(os.path.join(ROOT, "include", h), macro))


# ---- argument errors of sage_kvfork -------------------------------------------------------------------------------------------------
def _fork(lib, p, **kw):
    a = dict(k_int8=p, k_scale=p, v_image=p, v_scale=p, v_amax=p, k_mean=None, k_tail=p, v_tail=p, lens=p,
             block_table=p, bt_stride=2, num_pages=4, page_size=64, max_pages_per_seq=2, B=2, Hkv=1, head_dim=64, dtype=0,
             src_slots=p, dst_slots=p, new_pages=p, prefix_lens=None, n=1, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.sage_kvfork(*a.values()), lib.sage_last_error()


def test_argument_errors_do_not_need_a_gpu():
    lib = _cabi_kvfork.load()
    buf, p = _aligned_buffer()
    for name in ("k_int8", "k_scale", "v_image", "v_scale", "v_amax", "k_tail", "v_tail", "lens"):
        rc, msg = _fork(lib, p, **{name: None})
        assert rc == -1 and b"sage_kvfork: null cache pointer" in msg, (name, rc, msg)
    for name in ("src_slots", "dst_slots", "new_pages"):
        rc, msg = _fork(lib, p, **{name: None})
        assert rc == -1 and b"null src_slots / dst_slots / new_pages" in msg, (name, rc, msg)
    rc, msg = _fork(lib, p, block_table=None)
    assert rc == -1 and b"null block_table" in msg
    for ps in BAD_PAGE_SIZES:
        rc, msg = _fork(lib, p, page_size=ps)
        assert rc == -1 and b"page_size must be 64 * 2^k" in msg, (ps, msg)
    for n in (0, -1):
        rc, msg = _fork(lib, p, num_pages=n)
        assert rc == -1 and b"num_pages must be at least 1" in msg
    for kw in (dict(max_pages_per_seq=0), dict(max_pages_per_seq=-2), dict(max_pages_per_seq=2 ** 24 + 1), dict(page_size=2 ** 30, max_pages_per_seq=2),
               dict(bt_stride=1)):
        rc, msg = _fork(lib, p, **kw)
        assert rc == -1 and b"max_pages_per_seq must be at least 1" in msg, (kw, msg)
    for kw in (dict(B=0), dict(B=65536), dict(Hkv=0), dict(Hkv=65536)):
        rc, msg = _fork(lib, p, **kw)
        assert rc == -1 and b"B and Hkv" in msg, (kw, msg)
    for D in (0, 32, 96, 256):
        rc, msg = _fork(lib, p, head_dim=D)
        assert rc == -1 and b"head_dim must be 64 or 128" in msg
    for dt in (2, -1):
        rc, msg = _fork(lib, p, dtype=dt)
        assert rc == -1 and b"bad dtype" in msg
    for name in ("k_int8", "k_scale", "v_image", "k_tail", "v_tail", "k_mean"):
        rc, msg = _fork(lib, p, **{name: p + 4})
        assert rc == -1 and b"16-byte aligned" in msg, (name, rc, msg)
    rc, msg = _fork(lib, p, block_table=p + 2)
    assert rc == -1 and b"block_table must be 4-byte aligned" in msg
    for name in ("src_slots", "dst_slots", "new_pages", "prefix_lens"):
        rc, msg = _fork(lib, p, **{name: p + 2})
        assert rc == -1 and b"src_slots / dst_slots / new_pages / prefix_lens" in msg and b"4-byte aligned" in msg, (name, rc, msg)
    for n in (0, -1, 65536):
        rc, msg = _fork(lib, p, n=n)
        assert rc == -1 and b"n must be in [1, 65535]" in msg, (n, msg)
    with pytest.raises(ValueError, match="n must be in"):
        _cabi.check(rc, "sage_kvfork")
    del buf


def test_two_violations_report_the_earlier_check():
    """The order the header lists (tests/test_kv_entry_check_order_host.py's scheme)."""
    lib = _cabi_kvfork.load()
    buf, p = _aligned_buffer()
    checks = [(dict(k_int8=None), b"null cache pointer"),
              (dict(src_slots=None), b"null src_slots"),
              (dict(block_table=None), b"null block_table"),
              (dict(page_size=96), b"page_size must be 64 * 2^k"),
              (dict(num_pages=0), b"num_pages must be at least 1"),
              (dict(max_pages_per_seq=0), b"max_pages_per_seq must be at least 1"),
              (dict(B=0), b"B and Hkv"),
              (dict(head_dim=96), b"head_dim must be 64 or 128"),
              (dict(dtype=2), b"bad dtype"),
              (dict(v_image=p + 4), b"16-byte aligned"),
              (dict(block_table=p + 2), b"block_table must be 4-byte aligned"),
              (dict(new_pages=p + 2), b"4-byte aligned"),
              (dict(n=0), b"n must be in")]
    covered = set()
    for (i, (kw_i, match_i)), (j, (kw_j, _)) in itertools.combinations(enumerate(checks), 2):
        if set(kw_i) & set(kw_j):
            continue
        rc, msg = _fork(lib, p, **kw_i, **kw_j)
        assert rc == -1 and match_i in msg, (kw_i, kw_j, rc, msg)
        covered.add((i, j))
    assert all((i, i + 1) in covered for i in range(len(checks) - 1)), sorted(covered)
    del buf


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def _cache(seeded=True):
    c = PagedQuantizedKVCache.allocate(6, 128, 4, 2, 2, 64, torch.float16, "cpu")
    if seeded:
        c.seed(torch.zeros(4, 2, 64, dtype=torch.float16), torch.ones(4, 2, 64))
    return c


def test_fork_value_errors_before_any_work():
    with pytest.raises(ValueError, match="no statistics"):
        _cache(seeded=False).fork([0], [1], [2])
    c = _cache()
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    for args, kw, match in (
            (([4], [1], [2]), {}, r"src_slots must be slot indices in \[0, 4\)"),
            (([-1], [1], [2]), {}, "src_slots"),
            (([0], [4], [2]), {}, r"dst_slots must be slot indices in \[0, 4\)"),
            (([0], [-1], [2]), {}, "dst_slots"),
            (([0], [1], [6]), {}, r"new_pages must be page ids in \[0, 6\)"),
            (([0], [1], [-1]), {}, "new_pages"),
            (([0, 0], [1, 1], [2, 3]), {}, "dst_slots must be distinct"),
            (([0, 1], [1, 2], [2, 3]), {}, "disjoint"),
            (([0], [0], [2]), {}, "disjoint"),                                        # a source that is its destination
            (([0, 0], [1, 2], [3, 3]), {}, "new_pages must be distinct"),
            (([0, 0], [1], [2]), {}, "one length"),
            (([0], [1], [2, 3]), {}, "one length"),
            (([0], [1], [2]), dict(prefix_lens=[1, 2]), "one length"),
            (([], [], []), {}, "one length"),
            ((i32(), i32(), i32()), {}, "one length"),
            ((i32(0, 0), i32(1), i32(2)), {}, "one length"),
            ((0, [1], [2]), {}, "src_slots"),
            (([0.0], [1], [2]), {}, "src_slots"),
            (([True], [1], [2]), {}, "src_slots"),
            (([0], "1", [2]), {}, "dst_slots"),
            (([0], [1], None), {}, "new_pages"),
            ((torch.zeros(1), [1], [2]), {}, "src_slots"),                            # dtype
            ((torch.zeros(1, 1, dtype=torch.int32), [1], [2]), {}, "src_slots"),      # 1-D
            (([0], i32(1).to("meta"), [2]), {}, "dst_slots"),                         # device
            (([0], [1], [2]), dict(prefix_lens=[1.5]), "prefix_lens"),
            (([0], [1], [2]), dict(prefix_lens=torch.zeros(1)), "prefix_lens"),
            (([0], [1], [2]), dict(prefix_lens=5), "prefix_lens")):
        with pytest.raises(ValueError, match=match):
            c.fork(*args, **kw)
    assert c.lens.tolist() == [0, 0, 0, 0] and bool((c.block_table == -1).all())
    assert "multiple of 64" in PagedQuantizedKVCache.fork.__doc__                     # the prefix rounding is documented


# ---- the build ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_unit_holds_one_kernel_per_head_size_without_scratch():
    mk = open(os.path.join(ROOT, "sageattention_amd", "csrc", "Makefile")).read()
    assert "sage_kv_fork.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()        # (tests/test_build_resources.py reads SRCS)
    rep = tbr._resource_report("sage_kv_fork.hip")
    assert len(rep) == 2 and all("kvpaged_fork_kernel" in k for k in rep), sorted(rep)
    assert any("ILi128E" in k for k in rep) and any("ILi64E" in k for k in rep), sorted(rep)
    for name, res in rep.items():
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, (name, res)


# ---- ref_kvfork against cases written out by hand -------------------------------------------------------------------------------------
# B 6 slots, H 2, D 2 (the restatement does not look at D), 8 pages.  Every array counts up from a base of its own, so every byte says where it
# came from; slot 0 is the parent of every case, its table names pages 5, 2, 7 (ps 128: three pages, cap 384) or 5, 2, 7, 1, 6, 3 (ps 64).
RB, RH, RD, RNP = 6, 2, 2, 8


def _state(page_size, parent_len, parent_table, with_mean=True):
    tpp = page_size // 64
    ar = lambda shape, base, dt: (np.arange(int(np.prod(shape)), dtype=np.int64) * 7 + base).astype(dt).reshape(shape)
    return dict(k_int8=ar((RNP, RH, page_size, RD), 1, np.int8), k_scale=ar((RNP, RH, tpp * 4), 1000, np.int32),
                v_image=ar((RNP, RH, tpp, RD, 64), 3, np.uint8), v_scale=ar((RB, RH, RD), 2000, np.int32), v_amax=ar((RB, RH, RD), 3000, np.int32),
                k_mean=ar((RB, RH, RD), 4000, np.int16) if with_mean else None, k_tail=ar((RB, RH, 64, RD), 5000, np.int16),
                v_tail=ar((RB, RH, 64, RD), 6000, np.int16), lens=np.array([parent_len, 11, 22, 33, 44, 55], dtype=np.int32),
                block_table=np.array([list(parent_table)] + [[-7 - b] * len(parent_table) for b in range(1, RB)], dtype=np.int32))


def _expect(before, page_size, d, length, table, copied, tail_rows, s=0):
    """The state after one fork 0 -> d, from facts written by hand: the child's length, its table entries {index: id}, the (source page,
    destination page, tiles) copied, the tail rows copied; the per-slot statistics always follow.  Everything else is ``before``."""
    exp = {k: (None if v is None else v.copy()) for k, v in before.items()}
    exp["lens"][d] = length
    for idx, pid in table.items():
        exp["block_table"][d, idx] = pid
    for sp, dp, t in copied:
        exp["k_int8"][dp, :, :64 * t] = before["k_int8"][sp, :, :64 * t]
        exp["k_scale"][dp, :, :4 * t] = before["k_scale"][sp, :, :4 * t]
        exp["v_image"][dp, :, :t] = before["v_image"][sp, :, :t]
    for k in ("v_scale", "v_amax", "k_mean"):
        if exp[k] is not None:
            exp[k][d] = before[k][s]
    for k in ("k_tail", "v_tail"):
        exp[k][d, :, :tail_rows] = before[k][s, :, :tail_rows]
    return exp


def _same(got, exp, what):
    for k in ref_kvfork.KEYS:
        if exp[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:4].tolist())


T128, T64 = (5, 2, 7), (5, 2, 7, 1, 6, 3)
# (page size, parent's lens entry, prefix or None) -> (child's length, child's table entries, pages copied (src, dst, tiles), tail rows); new page 4, child slot 3
HAND = [
    # ---- the whole parent, pages of 128 keys (cap 384)
    ((128, 0, None), (0, {0: 4}, [], 0)),
    ((128, 1, None), (1, {0: 4}, [(5, 4, 1)], 1)),
    ((128, 63, None), (63, {0: 4}, [(5, 4, 1)], 63)),
    ((128, 64, None), (64, {0: 4}, [(5, 4, 1)], 0)),                  # a closed tile in an open page, empty tails
    ((128, 65, None), (65, {0: 4}, [(5, 4, 2)], 1)),
    ((128, 128, None), (128, {0: 5, 1: 4}, [], 0)),                   # ps: a page boundary, no copy
    ((128, 130, None), (130, {0: 5, 1: 4}, [(2, 4, 1)], 2)),          # ps + 2
    ((128, 257, None), (257, {0: 5, 1: 2, 2: 4}, [(7, 4, 1)], 1)),
    ((128, 384, None), (384, {0: 5, 1: 2, 2: 7}, [], 0)),             # cap: no entry left for the new page
    ((128, 1000, None), (384, {0: 5, 1: 2, 2: 7}, [], 0)),            # lens above cap: clamped
    ((128, -5, None), (0, {0: 4}, [], 0)),                            # lens below 0: clamped
    # ---- pages of 64 keys (cap 384)
    ((64, 0, None), (0, {0: 4}, [], 0)),
    ((64, 1, None), (1, {0: 4}, [(5, 4, 1)], 1)),
    ((64, 63, None), (63, {0: 4}, [(5, 4, 1)], 63)),
    ((64, 64, None), (64, {0: 5, 1: 4}, [], 0)),
    ((64, 65, None), (65, {0: 5, 1: 4}, [(2, 4, 1)], 1)),
    ((64, 66, None), (66, {0: 5, 1: 4}, [(2, 4, 1)], 2)),             # ps + 2
    ((64, 384, None), (384, dict(enumerate(T64)), [], 0)),
    # ---- prefixes of the parent of 257 keys
    ((128, 257, 64), (64, {0: 4}, [(5, 4, 1)], 0)),
    ((128, 257, 100), (64, {0: 4}, [(5, 4, 1)], 0)),                  # below L, inside a block: rounded down
    ((128, 257, 128), (128, {0: 5, 1: 4}, [], 0)),
    ((128, 257, 200), (192, {0: 5, 1: 4}, [(2, 4, 1)], 0)),
    ((128, 257, 256), (256, {0: 5, 1: 2, 2: 4}, [], 0)),
    ((128, 257, 257), (257, {0: 5, 1: 2, 2: 4}, [(7, 4, 1)], 1)),     # at L: not rounded
    ((128, 257, 262), (257, {0: 5, 1: 2, 2: 4}, [(7, 4, 1)], 1)),     # above L: clamped to L
    ((128, 257, 2 ** 31 - 1), (257, {0: 5, 1: 2, 2: 4}, [(7, 4, 1)], 1)),
    ((128, 257, 0), (0, {0: 4}, [], 0)),
    ((128, 257, 63), (0, {0: 4}, [], 0)),
    ((128, 257, -3), (0, {0: 4}, [], 0)),                             # negative: clamped to 0
    ((128, 257, -2 ** 31), (0, {0: 4}, [], 0)),
    ((64, 257, 100), (64, {0: 5, 1: 4}, [], 0)),
    ((64, 257, 256), (256, {0: 5, 1: 2, 2: 7, 3: 1, 4: 4}, [], 0)),
    ((64, 130, 130), (130, {0: 5, 1: 2, 2: 4}, [(7, 4, 1)], 2)),
]


@pytest.mark.parametrize("case", range(len(HAND)), ids=[f"ps{ps}-len{n}-prefix{p}" for (ps, n, p), _ in HAND])
def test_ref_gives_the_hand_written_result(case):
    (ps, n, prefix), (length, table, copied, tail_rows) = HAND[case]
    for with_mean in (True, False):
        before = _state(ps, n, T128 if ps == 128 else T64, with_mean)
        got = ref_kvfork.fork_state(before, ps, [0], [3], [4], None if prefix is None else [prefix])
        _same(got, _expect(before, ps, 3, length, table, copied, tail_rows), HAND[case][0])
    assert ref_kvfork.prefix_len(min(max(n, 0), 384), prefix) == length


def test_ref_skips_bad_slots_and_does_not_write_the_pool_through_bad_pages():
    before = _state(128, 130, T128)
    for s, d in ((-1, 3), (RB, 3), (0, -1), (0, RB), (2, 2), (0, 0), (2 ** 31 - 1, 3), (0, -2 ** 31)):
        _same(ref_kvfork.fork_state(before, 128, [s], [d], [4]), before, (s, d))              # skipped entirely
    for pg in (-1, RNP, 2 ** 31 - 1, -2 ** 31):                                                 # the table takes it as given, the pool nothing
        _same(ref_kvfork.fork_state(before, 128, [0], [3], [pg]), _expect(before, 128, 3, 130, {0: 5, 1: pg}, [], 2), pg)
    for sp in (-1, RNP, 2 ** 31 - 1):                                                           # the parent's open page is no page of the pool
        b2 = {k: (None if v is None else v.copy()) for k, v in before.items()}
        b2["block_table"][0, 1] = sp
        _same(ref_kvfork.fork_state(b2, 128, [0], [3], [4]), _expect(b2, 128, 3, 130, {0: 5, 1: 4}, [], 2), sp)
    # a bad id in a shared entry is copied as it stands
    b2 = {k: (None if v is None else v.copy()) for k, v in before.items()}
    b2["block_table"][0, 0] = -1
    _same(ref_kvfork.fork_state(b2, 128, [0], [3], [4]), _expect(b2, 128, 3, 130, {0: -1, 1: 4}, [(2, 4, 1)], 2), "shared -1")


def test_ref_many_forks_of_one_call():
    """One source to two destinations, a second source, a skipped fork between them: each as if alone."""
    before = _state(128, 130, T128)
    before["lens"][1] = 63
    before["block_table"][1] = (6, -9, -9)
    got = ref_kvfork.fork_state(before, 128, [0, 0, 9, 1], [3, 4, 5, 2], [4, 1, 0, 3], [130, 64, 5, 70])
    exp = _expect(before, 128, 3, 130, {0: 5, 1: 4}, [(2, 4, 1)], 2)
    exp = _expect(exp, 128, 4, 64, {0: 1}, [(5, 1, 1)], 0)
    exp = _expect(exp, 128, 2, 63, {0: 3}, [(6, 3, 1)], 63, s=1)
    _same(got, exp, "four forks")
    assert got["lens"].tolist() == [130, 63, 63, 130, 64, 55]
