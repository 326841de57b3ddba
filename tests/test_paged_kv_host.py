"""CPU: the paged KV cache's C boundary, Python interface and build (include/sage_kvpaged_gfx950.h, sageattention_amd/_cabi_kvpaged.py,
sageattention_amd/paged_kv_cache.py, csrc/sage_attn_d{128,64}_{f8p,f8pg}.hip).  The new header's prototypes are the new binding's table, the
library exports them, every argument error returns -1 with its message before anything touches a GPU, the Python layer raises ValueError
before any work, each new unit holds exactly the paged kernels of the forms of the unit lists it is instantiated from, without scratch -- and
none of it moved what the main header, the contiguous cache's header, their bindings and the package's ``__all__`` pin."""
import ctypes
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import util  # noqa: F401  (sys.path)
import sageattention_amd as sa
import test_build_resources as tbr
from sageattention_amd import _cabi, _cabi_kvcache, _cabi_kvpaged
from sageattention_amd.kv_cache import sageattn_kvcache
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
from test_kv_cache_host import MAIN_HEADER, _ctype_of, _prototypes, _text

kf = tbr.kf
ROOT = tbr.ROOT
CSRC = os.path.join(ROOT, "sageattention_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "sage_kvpaged_gfx950.h")
KVCACHE_HEADER = os.path.join(ROOT, "include", "sage_kvcache_gfx950.h")
ENTRIES = ["sage_kvpaged_abi_version", "sage_kvpaged_append", "sage_kvpaged_attn"]


def _ctype(ctype):
    return ctypes.c_void_p if ctype.endswith("*") else _ctype_of(ctype)


def test_binding_is_the_header():
    protos = _prototypes(HEADER, "SAGE_KVPAGED_API")
    assert sorted(protos) == sorted(_cabi_kvpaged.SYMBOLS) == ENTRIES
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_kvpaged.SYMBOLS[name]
        assert res is _ctype(ret), f"{name}: returns {ret}, bound as {res}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters declared, {len(argtypes)} bound"
        for i, (ctype, bound) in enumerate(zip(params, argtypes)):
            assert bound is _ctype(ctype), f"{name}: parameter {i} ({ctype}) bound as {bound}"
    version = int(re.search(r"#define\s+SAGE_KVPAGED_ABI_VERSION\s+(\d+)", _text(HEADER)).group(1))
    assert version == 1 == _cabi_kvpaged.ABI_VERSION
    rest = re.sub(r"SAGE_KVPAGED_API", "", _text(HEADER))
    assert "SAGE_API" not in rest and "SAGE_KVCACHE_API" not in rest          # an export macro of its own


def test_library_exports_the_entries():
    lib = ctypes.CDLL(_cabi.LIB_PATH)
    for name in _cabi_kvpaged.SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
    assert _cabi_kvpaged.load() is _cabi.load()                      # one library, bound behind _cabi.load()
    assert _cabi_kvpaged.load().sage_kvpaged_abi_version() == 1


def test_existing_boundaries_did_not_move():
    lib = _cabi.load()
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22
    assert len(_prototypes(MAIN_HEADER, "SAGE_API")) == 56 and len(_cabi.SYMBOLS) == 56
    assert sorted(_prototypes(KVCACHE_HEADER, "SAGE_KVCACHE_API")) == sorted(_cabi_kvcache.SYMBOLS) == ["sage_kvcache_abi_version", "sage_kvcache_append"]
    assert _cabi_kvcache.ABI_VERSION == 1 and _cabi_kvcache.load().sage_kvcache_abi_version() == 1
    assert not any(n.startswith("sage_kvpaged") for n in list(_cabi.SYMBOLS) + list(_cabi_kvcache.SYMBOLS))
    assert sorted(sa.__all__) == sorted(["sageattn", "sageattn_varlen", "sageattn_qk_int8_pv_fp16_triton", "sageattn_qk_int8_pv_fp16_cuda",
                                         "sageattn_qk_int8_pv_fp8_cuda", "sageattn_qk_int8_pv_fp8_cuda_sm90", "sageattn_qk_int8_pv_fp8_varlen"])
    assert not hasattr(sa, "PagedQuantizedKVCache")


# ---- argument errors of the two entries ----------------------------------------------------------------------------------------------
def _append(lib, p, **kw):
    a = dict(k_int8=p, k_scale=p, v_image=p, v_scale=p, v_amax=p, k_mean=None, k_tail=p, v_tail=p, lens=p, k_new=p, v_new=p, new_lens=None,
             B=1, Hkv=1, T=1, head_dim=64, k_sb=64, k_sh=64, k_sl=64, v_sb=64, v_sh=64, v_sl=64, dtype=0,
             block_table=p, bt_stride=2, num_pages=4, page_size=64, max_pages_per_seq=2, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.sage_kvpaged_append(*a.values()), lib.sage_last_error()


def _attn(lib, p, attr=None, **kw):
    a = dict(q=p, k_int8=p, v_image=p, o=p, lse=None, k_scale=p, v_scale=p, kv_lens=p, block_table=p, bt_stride=2, num_pages=4, page_size=64,
             max_pages_per_seq=2, B=1, Hq=2, Hkv=1, Lq=1, D=64, q_sb=128, q_sh=64, q_sl=64, k_sb=4096, k_sh=4096, k_sl=64, o_sb=128, o_sh=64, o_sl=64,
             is_causal=0, sm_scale_log2=1.0, q_dtype=0, out_dtype=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.sage_kvpaged_attn(*a.values(), _cabi.attr_arg(attr)), lib.sage_last_error()


def _aligned_buffer():
    buf = ctypes.create_string_buffer(4096)
    return buf, (ctypes.addressof(buf) + 127) & ~127


BAD_PAGE_SIZES = (0, -64, 32, 63, 96, 100, 192, 320)


def test_append_argument_errors_do_not_need_a_gpu():
    lib = _cabi_kvpaged.load()
    buf, p = _aligned_buffer()
    for name in ("k_int8", "k_scale", "v_image", "v_scale", "v_amax", "k_tail", "v_tail", "lens"):
        rc, msg = _append(lib, p, **{name: None})
        assert rc == -1 and b"null cache pointer" in msg, (name, rc, msg)
    for name in ("k_new", "v_new"):
        rc, msg = _append(lib, p, **{name: None})
        assert rc == -1 and b"null k_new / v_new" in msg, (name, rc, msg)
    rc, msg = _append(lib, p, block_table=None)
    assert rc == -1 and b"null block_table" in msg
    for ps in BAD_PAGE_SIZES:
        rc, msg = _append(lib, p, page_size=ps)
        assert rc == -1 and b"page_size must be 64 * 2^k" in msg, (ps, msg)
    for n in (0, -1):
        rc, msg = _append(lib, p, num_pages=n)
        assert rc == -1 and b"num_pages must be at least 1" in msg
    for kw in (dict(max_pages_per_seq=0), dict(max_pages_per_seq=-2), dict(max_pages_per_seq=2 ** 24 + 1), dict(page_size=2 ** 30, max_pages_per_seq=2),
               dict(bt_stride=1)):
        rc, msg = _append(lib, p, **kw)
        assert rc == -1 and b"max_pages_per_seq must be at least 1" in msg, (kw, msg)
    for kw in (dict(B=0), dict(B=65536), dict(Hkv=0), dict(Hkv=65536)):
        rc, msg = _append(lib, p, **kw)
        assert rc == -1 and b"B and Hkv" in msg, (kw, msg)
    for D in (0, 32, 96, 256):
        rc, msg = _append(lib, p, head_dim=D)
        assert rc == -1 and b"head_dim must be 64 or 128" in msg
    for T in (0, -3):
        rc, msg = _append(lib, p, T=T)
        assert rc == -1 and b"T must be at least 1" in msg
    for name in ("k_int8", "k_scale", "v_image", "k_tail", "v_tail", "k_new", "v_new", "k_mean"):
        rc, msg = _append(lib, p, **{name: p + 2})
        assert rc == -1 and b"16-byte aligned" in msg, (name, rc, msg)
    rc, msg = _append(lib, p, block_table=p + 2)
    assert rc == -1 and b"block_table must be 4-byte aligned" in msg
    for name in ("k_sb", "k_sh", "k_sl", "v_sb", "v_sh", "v_sl"):
        rc, msg = _append(lib, p, **{name: 68})
        assert rc == -1 and b"multiples of 8 elements" in msg, (name, rc, msg)
    rc, msg = _append(lib, p, dtype=2)
    assert rc == -1 and b"dtype" in msg
    with pytest.raises(ValueError, match="dtype"):
        _cabi.check(rc, "sage_kvpaged_append")
    del buf


def test_attention_argument_errors_do_not_need_a_gpu():
    lib = _cabi_kvpaged.load()
    buf, p = _aligned_buffer()
    for name in ("q", "k_int8", "v_image", "o", "k_scale", "v_scale"):
        rc, msg = _attn(lib, p, **{name: None})
        assert rc == -1 and b"null tensor pointer" in msg, (name, rc, msg)
    for name in ("kv_lens", "block_table"):
        rc, msg = _attn(lib, p, **{name: None})
        assert rc == -1 and b"null " + name.encode() in msg, (name, rc, msg)
    for ps in BAD_PAGE_SIZES:
        rc, msg = _attn(lib, p, page_size=ps)
        assert rc == -1 and b"page_size must be 64 * 2^k" in msg, (ps, msg)
    rc, msg = _attn(lib, p, num_pages=0)
    assert rc == -1 and b"num_pages must be at least 1" in msg
    for kw in (dict(max_pages_per_seq=0), dict(page_size=2 ** 30, max_pages_per_seq=2), dict(bt_stride=1)):
        rc, msg = _attn(lib, p, **kw)
        assert rc == -1 and b"max_pages_per_seq must be at least 1" in msg, (kw, msg)
    for kw in (dict(B=0), dict(B=65536), dict(Hkv=0), dict(Hkv=65536)):
        rc, msg = _attn(lib, p, **kw)
        assert rc == -1 and b"B and Hkv" in msg, (kw, msg)
    for D in (0, 32, 96, 256):
        rc, msg = _attn(lib, p, D=D)
        assert rc == -1 and b"head_dim must be 64 or 128" in msg
    for kw, match in ((dict(Lq=0), b"empty problem"), (dict(Hq=3, Hkv=2), b"divisible"), (dict(q=p + 2), b"16-byte aligned"), (dict(k_int8=p + 4), b"16-byte aligned"),
                      (dict(q_sl=68), b"q strides"), (dict(k_sl=72), b"k strides"), (dict(o_sh=4), b"output strides"), (dict(q_dtype=2), b"q_dtype"),
                      (dict(out_dtype=-1), b"out_dtype")):
        rc, msg = _attn(lib, p, **kw)
        assert rc == -1 and match in msg, (kw, rc, msg)
    # what a paged call does not take, each refused by name
    ws = type("ws", (), dict(data_ptr=lambda s: p, numel=lambda s: 4096, element_size=lambda s: 1))()
    for attr, match in ((_cabi.launch_attr(ws, kv_split=2), b"SAGE_ATTR_KV_SPLIT is not supported on a paged cache"),
                        (_cabi.launch_attr(folded_scores=True), b"SAGE_ATTR_FP8_FOLDED_SCORES is not supported on a paged cache"),
                        (_cabi.launch_attr(ws, force_persistent=True), b"SAGE_ATTR_FORCE_PERSISTENT is not supported on a paged cache")):
        rc, msg = _attn(lib, p, attr=attr)
        assert rc == -1 and match in msg, (rc, msg)
    # ... and what it takes as the kv_lens entry does keeps that entry's conditions
    rc, msg = _attn(lib, p, attr=_cabi.launch_attr(window=5))
    assert rc == -1 and b"SageLaunchAttr.window" in msg
    rc, msg = _attn(lib, p, attr=_cabi.launch_attr(gqa_pack=True), Lq=33)
    assert rc == -1 and b"SAGE_ATTR_GQA_PACK" in msg
    del buf


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
def _cache(dtype=torch.float16, seeded=True, smooth=True):
    c = PagedQuantizedKVCache.allocate(6, 128, 2, 2, 2, 64, dtype, "cpu")
    if seeded:
        c.seed(torch.zeros(2, 2, 64, dtype=dtype) if smooth else None, torch.ones(2, 2, 64))
    return c


def test_allocate_shapes_and_errors():
    c = _cache(seeded=False)
    assert (c.num_pages, c.page_size, c.B, c.max_pages_per_seq, c.Hkv, c.D, c.dtype, c.capacity) == (6, 128, 2, 2, 2, 64, torch.float16, 256)
    assert c.k_int8.shape == (6, 2, 128, 64) and c.k_int8.dtype == torch.int8
    assert c.k_scale.shape == (6, 2, 8) and c.k_scale.dtype == torch.float32
    assert c.v_image.shape == (6, 2, 2, 64, 64) and c.v_image.dtype == torch.uint8
    assert c.v_scale.shape == c.v_amax.shape == (2, 2, 64) and c.k_mean.shape == (2, 2, 64) and c.k_mean.dtype == torch.float16
    assert c.k_tail.shape == c.v_tail.shape == (2, 2, 64, 64) and c.lens.tolist() == [0, 0] and c.lens.dtype == torch.int32
    assert c.block_table.shape == (2, 2) and c.block_table.dtype == torch.int32 and c.block_table.tolist() == [[-1, -1], [-1, -1]]
    assert all(t.is_contiguous() for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail, c.lens, c.block_table))
    for bad in (dict(D=96), dict(B=0), dict(Hkv=0), dict(num_pages=0), dict(max_pages_per_seq=0), dict(dtype=torch.float32), dict(page_size=96),
                dict(page_size=32), dict(page_size=0), dict(page_size=192), dict(page_size=64.0), dict(num_pages=True),
                dict(page_size=2 ** 20, max_pages_per_seq=2 ** 11)):
        kw = dict(num_pages=4, page_size=64, B=2, max_pages_per_seq=2, Hkv=2, D=64, dtype=torch.float16, device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError):
            PagedQuantizedKVCache.allocate(**kw)


def test_seed_errors_state_and_slots():
    c = _cache(seeded=False)
    with pytest.raises(ValueError, match="k_mean"):
        c.seed(torch.zeros(2, 2, 64), torch.ones(2, 2, 64))                              # dtype
    with pytest.raises(ValueError, match="v_amax"):
        c.seed(None, torch.ones(2, 64))
    with pytest.raises(ValueError, match="seeded cache"):
        c.seed(None, torch.ones(1, 2, 64), slots=[1])                                    # slots of a cache that was never seeded
    km = torch.full((2, 2, 64), 0.5, dtype=torch.float16)
    c.lens.fill_(7)
    assert c.seed(km, torch.full((2, 2, 64), 3.0, dtype=torch.float64)) is c
    assert c.lens.tolist() == [0, 0] and torch.equal(c.k_mean, km) and bool((c.v_amax == 3.0).all())
    # one slot: its statistics and its length alone
    c.lens.copy_(torch.tensor([5, 9], dtype=torch.int32))
    table = c.block_table.clone()
    assert c.seed(torch.full((1, 2, 64), 2.0, dtype=torch.float16), torch.full((1, 2, 64), 4.0), slots=[1]) is c
    assert c.lens.tolist() == [5, 0] and bool((c.k_mean[0] == 0.5).all()) and bool((c.k_mean[1] == 2.0).all())
    assert bool((c.v_amax[0] == 3.0).all()) and bool((c.v_amax[1] == 4.0).all()) and torch.equal(c.block_table, table)
    c.seed(torch.full((2, 2, 64), 1.0, dtype=torch.float16), torch.full((2, 2, 64), 6.0), slots=torch.tensor([1, 0]))
    assert c.lens.tolist() == [0, 0] and bool((c.k_mean == 1.0).all()) and bool((c.v_amax == 6.0).all())
    for kw, match in ((dict(k_mean=None, v_amax=torch.ones(1, 2, 64), slots=[0]), "k_mean must be a tensor"),          # None-ness differs from the cache's
                      (dict(k_mean=km[:1], v_amax=torch.ones(2, 2, 64), slots=[0]), "v_amax"),                         # [len(slots), Hkv, D]
                      (dict(k_mean=km, v_amax=torch.ones(1, 2, 64), slots=[0]), "k_mean"),
                      (dict(k_mean=km[:1], v_amax=torch.ones(1, 2, 64), slots=[2]), "slots"),
                      (dict(k_mean=km, v_amax=torch.ones(2, 2, 64), slots=[0, 0]), "slots"),
                      (dict(k_mean=km[:1], v_amax=torch.ones(1, 2, 64), slots=[True]), "slots"),
                      (dict(k_mean=km[:1], v_amax=torch.ones(1, 2, 64), slots=1), "slots"),
                      (dict(k_mean=km[:1], v_amax=torch.ones(1, 2, 64), slots=torch.zeros(1)), "slots")):
        with pytest.raises(ValueError, match=match):
            c.seed(**kw)
    assert c.lens.tolist() == [0, 0] and bool((c.v_amax == 6.0).all())
    plain = _cache(smooth=False)
    assert plain.k_mean is None
    with pytest.raises(ValueError, match="k_mean must be None"):
        plain.seed(km[:1], torch.ones(1, 2, 64), slots=[0])
    plain.seed(None, torch.full((1, 2, 64), 2.0), slots=[1])
    assert plain.k_mean is None and bool((plain.v_amax[1] == 2.0).all()) and bool((plain.v_amax[0] == 1.0).all())


def test_append_value_errors_before_any_work():
    h = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt)
    with pytest.raises(ValueError, match="no statistics"):
        _cache(seeded=False).append(h(2, 2, 1, 64), h(2, 2, 1, 64))
    c = _cache()
    for k_new, v_new, kw, match in (
            (h(2, 2, 1, 64, dt=torch.bfloat16), h(2, 2, 1, 64, dt=torch.bfloat16), {}, "dtype"),
            (h(2, 2, 1, 64), h(2, 2, 2, 64), {}, "one shape"),
            (h(3, 2, 1, 64), h(3, 2, 1, 64), {}, "B, Hkv, D"),
            (h(2, 2, 1, 128), h(2, 2, 1, 128), {}, "B, Hkv, D"),
            (h(2, 2, 1, 64), h(2, 2, 1, 64), dict(tensor_layout="NHD"), "B, Hkv, D"),
            (h(2, 2, 0, 64), h(2, 2, 0, 64), {}, "at least one row"),
            (h(2, 2, 64), h(2, 2, 64), {}, "4-D"),
            (h(2, 2, 1, 64), h(2, 2, 1, 64), dict(tensor_layout="HDN"), "layout"),
            (h(2, 2, 1, 64), h(2, 2, 1, 64), dict(new_lens=torch.zeros(2)), "new_lens"),
            (h(2, 2, 1, 64), h(2, 2, 1, 64), dict(new_lens=torch.zeros(3, dtype=torch.int32)), "new_lens"),
            (h(2, 2, 1, 64).to("meta"), h(2, 2, 1, 64).to("meta"), {}, "device")):
        with pytest.raises(ValueError, match=match):
            c.append(k_new, v_new, **kw)
    assert c.lens.tolist() == [0, 0]


def test_attention_value_errors_before_any_work():
    """The cache's own checks, ``num_splits`` on a paged cache, and the keywords' ValueErrors of the family's one resolver."""
    c = _cache()
    q = torch.zeros(2, 4, 1, 64, dtype=torch.float16)
    for args, kw, match in (
            ((q.float(), c), {}, "dtype"),
            ((q.to("meta"), c), {}, "device"),
            ((torch.zeros(3, 4, 1, 64, dtype=torch.float16), c), {}, "B, D"),
            ((torch.zeros(2, 3, 1, 64, dtype=torch.float16), c), {}, "divisible"),
            ((q, "cache"), {}, "PagedQuantizedKVCache"),
            ((q, _cache(seeded=False)), {}, "no statistics"),
            ((q, c), dict(tensor_layout="HDN"), "layout"),
            ((q, c), dict(num_splits=2), "num_splits is not supported on a PagedQuantizedKVCache"),
            ((q, c), dict(num_splits="auto"), "num_splits is not supported on a PagedQuantizedKVCache"),
            ((q, c), dict(num_splits=1), "num_splits is not supported on a PagedQuantizedKVCache"),
            ((q, c), dict(num_splits=0, pack_gqa=1), "num_splits is not supported"),          # the earlier keyword's error
            ((q, c), dict(causal_align="middle"), "causal_align"),
            ((q, c), dict(causal_align="bottom_right"), "needs is_causal=True"),
            ((q, c), dict(q_start=1), "needs is_causal=True"),
            ((q, c), dict(is_causal=True, q_start=1, causal_align="bottom_right"), "not both"),
            ((q, c), dict(is_causal=True, q_start=torch.zeros(3, dtype=torch.int32)), r"shape \[B\]"),
            ((q, c), dict(window_size=(70,)), "window_size"),
            ((q, c), dict(is_causal=True, window_size=(70, 5)), "window_size"),
            ((q, c), dict(pack_gqa=1), "pack_gqa"),
            ((q, c), dict(pack_gqa=1, window_size=(70,)), "pack_gqa"),                        # the resolver's order: pack_gqa before window_size
            ((torch.zeros(2, 4, 33, 64, dtype=torch.float16), c), dict(pack_gqa=True), "qo_len <= 32"),
            ((torch.zeros(2, 2, 1, 64, dtype=torch.float16), c), dict(pack_gqa=True), "no GQA group")):
        with pytest.raises(ValueError, match=match):
            sageattn_kvcache(*args, **kw)


def test_from_prefill_value_errors():
    k = torch.zeros(2, 2, 8, 64, dtype=torch.float16)
    long = torch.zeros(2, 2, 200, 64, dtype=torch.float16)
    t = torch.zeros(2, 2, dtype=torch.int32)
    for args, kw in (((k, k[:, :, :4], t, 4, 64), {}), ((k, k.bfloat16(), t, 4, 64), {}), ((k[0], k[0], t, 4, 64), {}), ((k, k, t, 4, 64), dict(v_headroom=0.0)),
                     ((k, k, t, 4, 64), dict(kv_lens=torch.zeros(3, dtype=torch.int32))), ((k, k, t, 4, 64), dict(tensor_layout="HDN")),
                     ((k, k, t.float(), 4, 64), {}), ((k, k, t[:1], 4, 64), {}), ((k, k, t[0], 4, 64), {}), ((k, k, [[0, 1], [2, 3]], 4, 64), {}),
                     ((k, k, t, 4, 96), {}), ((k, k, t, 0, 64), {}),
                     ((long, long, t, 4, 64), {})):        # 200 rows do not fit into two pages of 64
        with pytest.raises(ValueError):
            PagedQuantizedKVCache.from_prefill(*args, **kw)


# ---- the build --------------------------------------------------------------------------------------------------------------------------
# Each new unit holds exactly the paged kernels of the forms of the lists it names (read from the header with a small host program, as
# tests/test_kernel_form.py does), every kernel without scratch and at the occupancy of its form.
PAGED_UNITS = {"f8p": ("UNIT_F8K", "UNIT_F8Q", "UNIT_F8W"), "f8pg": ("UNIT_F8G",)}
PROGRAM = r"""
#include "sage_attn_form.h"
#include <cstdio>
using namespace sage;
int main()
{
    const AttnUnit units[] = {UNIT_F8K, UNIT_F8Q, UNIT_F8W, UNIT_F8G};
    const char *names[] = {"UNIT_F8K", "UNIT_F8Q", "UNIT_F8W", "UNIT_F8G"};
    for (int u = 0; u < 4; u++)
        for (int D : {128, 64}) {
            const FormList l = unit_forms(units[u], D);
            for (int i = 0; i < l.n; i++) printf("%s %d %u %d\n", names[u], D, l.v[i], min_waves(unpack(l.v[i])));
        }
    return 0;
}
"""


@pytest.fixture(scope="module")
def listed(tmp_path_factory):
    """{(unit name, D): {packed form: min_waves}} of the four lists the paged units are instantiated from"""
    tmp = tmp_path_factory.mktemp("paged_forms")
    src, exe = tmp / "forms.hip", tmp / "forms"
    src.write_text(PROGRAM)
    out = subprocess.run([tbr.HIPCC, "-std=c++17", "--cuda-host-only", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lists = {}
    for line in run.stdout.strip().split("\n"):
        unit, D, word, waves = line.split()
        lists.setdefault((unit, int(D)), {})[int(word)] = int(waves)
    return lists


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_paged_units_hold_the_paged_kernels_of_their_lists_without_scratch(listed):
    srcs = [f"sage_attn_d{D}_{u}.hip" for u in PAGED_UNITS for D in (128, 64)]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert all(s in re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split() for s in srcs + ["sage_kv_paged.hip", "sage_kv_cache.hip"])
    with ThreadPoolExecutor(max_workers=len(srcs)) as ex:
        reports = dict(zip(srcs, ex.map(tbr._resource_report, srcs)))
    for u, units in PAGED_UNITS.items():
        for D in (128, 64):
            rep = reports[f"sage_attn_d{D}_{u}.hip"]
            want = {}
            for unit in units:
                want.update(listed[(unit, D)])
            assert len(want) == 8
            assert not [k for k in rep if "sage_attn_kernel" in k], "an unpaged kernel in a paged unit"
            mine = {k: v for k, v in rep.items() if "sage_attn_paged_kernel" in k}
            assert {kf.pack(kf.decode_paged(k)) for k in mine} == set(want) and len(mine) == 8, (u, D, sorted(mine))
            for name, res in mine.items():
                f = kf.decode_paged(name)
                assert f["D"] == D and f["kvlen"] and not f["seed"] and kf.encode_paged(f) == name
                assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0, (name, res)
                assert res["Occupancy"] >= want[kf.pack(f)], (name, res)
    # the names are two families: neither helper reads the other's
    some = next(k for k in reports["sage_attn_d64_f8pg.hip"] if "sage_attn_paged_kernel" in k)
    with pytest.raises(ValueError):
        kf.decode(some)
    with pytest.raises(ValueError):
        kf.decode_paged(kf.encode(kf.decode_paged(some)))


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_cache_units_use_no_scratch():
    for src, kernels in (("sage_kv_cache.hip", ("kvcache_append_kernel", "kvcache_commit_kernel")), ("sage_kv_paged.hip", ("kvpaged_append_kernel",))):
        rep = tbr._resource_report(src)
        for kname in kernels:
            assert any(kname in k for k in rep), (src, kname)
        assert len(rep) == (5 if src == "sage_kv_cache.hip" else 4), (src, sorted(rep))
        for name, res in rep.items():
            assert res.get("ScratchSize", 0) == 0 and res.get("VGPRs Spill", 0) == 0, (src, name, res)
