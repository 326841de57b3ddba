"""CPU: the C boundary and Python interface of the appendable quantised latent of the absorbed MLA decode route
(include/sage_mlacache_gfx950.h, sageattention_amd/_cabi_mlacache.py, sageattention_amd/mla_cache.py).  The header's prototypes are the binding's
table; both entries refuse bad arguments with -1 and their message, in the header's order, before anything touches a GPU (host memory only);
the Python layer raises ValueError before any work; none of the pinned symbol tables or the package's public names moved."""
import os
import re

import pytest
import torch

import util  # noqa: F401  (sys.path)
import test_paged_kv_host as paged
from test_kv_cache_host import _prototypes
from sageattention_amd import _cabi, _cabi_mla, _cabi_mlacache, _cabi_mlasplit
from sageattention_amd.mla_cache import MlaLatentCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sage_mlacache_gfx950.h")
F16, BF16 = torch.float16, torch.bfloat16


def test_binding_is_the_header_and_nothing_else_moved():
    import sageattention_amd as sa
    protos = _prototypes(HEADER, "SAGE_MLACACHE_API")
    assert sorted(protos) == sorted(_cabi_mlacache.SYMBOLS) == ["sage_mlacache_abi_version", "sage_mlacache_append", "sage_mlacache_stats"]
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_mlacache.SYMBOLS[name]
        assert res is paged._ctype(ret) and [paged._ctype(c) for c in params] == list(argtypes), name
    lib = _cabi_mlacache.load()
    assert lib is _cabi.load() and lib.sage_mlacache_abi_version() == _cabi_mlacache.ABI_VERSION == 1
    assert "#define SAGE_MLACACHE_ABI_VERSION 1" in open(HEADER).read()
    assert sorted(_cabi_mla.SYMBOLS) == ["sage_mla_abi_version", "sage_mla_attn", "sage_mla_prepass", "sage_mla_ws_floats"]
    assert sorted(_cabi_mlasplit.SYMBOLS) == ["sage_mlasplit_abi_version", "sage_mlasplit_attn", "sage_mlasplit_ws_bytes"]
    assert len(_cabi.SYMBOLS) == 56 and not any(n.startswith("sage_mla") for n in _cabi.SYMBOLS)
    assert not any("mla" in n.lower() for n in sa.__all__) and not hasattr(sa, "MlaLatentCache")
    mk = open(os.path.join(ROOT, "sageattention_amd", "csrc", "Makefile")).read()
    assert "sage_mla_cache.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert "../../include/sage_mlacache_gfx950.h" in re.search(r"^HDRS\s*:=\s*(.*)$", mk, re.M).group(1).split()


def _args(entry, p, **kw):
    a = (dict(kv=p, kv_lens=None, k_mean=p, v_amax=p, ws=p, ws_floats=1600, B=1, Lk=1, kv_sb=576, kv_sl=576, smooth_k=1, dtype=1, stream=None)
         if entry == "stats" else
         dict(kv_new=p, new_lens=None, lens=p, tail=p, k_mean=p, v_amax=p, k_image=p, k_scale=p, v_image=p, v_scale=p, B=1, T=1, capacity=64,
              kvn_sb=576, kvn_sl=576, smooth_k=1, dtype=0, stream=None))
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("entry,bad,message", [             # the header's order: each case is good in everything in front of it
    ("stats", dict(dtype=2, B=0), b"dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got 2)"),
    ("stats", dict(Lk=0, kv=None), b"empty problem (B 1, Lk 0)"),
    ("stats", dict(v_amax=None, kv_sl=8), b"null pointer (only kv_lens may be null)"),
    ("stats", dict(kv_sl=568, k_mean="+1"), b"kv must be 16-byte aligned with non-negative strides in multiples of 8 elements and a token stride"),
    ("stats", dict(k_mean="+1", ws_floats=0), b"v_amax, ws and kv_lens must be 4-byte aligned, k_mean 2-byte"),
    ("stats", dict(ws_floats=1599, B=1 << 20), b"ws holds 1599 floats, sage_mla_ws_floats(B, Lk) = "),
    ("stats", dict(B=65536, ws_floats=1 << 40), b"B must be at most 65535 (got 65536)"),
    ("append", dict(dtype=-1, T=0), b"dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got -1)"),
    ("append", dict(T=0, lens=None), b"empty problem (B 1, T 0, capacity 64)"),
    ("append", dict(tail=None, kvn_sl=8), b"null pointer (only new_lens may be null)"),
    ("append", dict(kvn_sb=-576, v_scale="+2"), b"kv_new must be 16-byte aligned with non-negative strides"),
    ("append", dict(new_lens="+2", B=65536), b"tail and the images must be 16-byte aligned, k_scale, v_scale, v_amax, lens and new_lens 4-byte"),
    ("append", dict(B=65536), b"B must be at most 65535, T and capacity at most 2^30 (got 65536, 1 and 64)"),
])
def test_the_entries_refuse_with_their_message(entry, bad, message):
    lib = _cabi_mlacache.load()
    buf, p = paged._aligned_buffer()
    bad = {n: (p + int(x) if isinstance(x, str) else x) for n, x in bad.items()}       # "+n": the aligned address plus n bytes
    assert getattr(lib, "sage_mlacache_" + entry)(*_args(entry, p, **bad)) == -1
    err = lib.sage_last_error()
    assert err.startswith(b"sage_mlacache_" + entry.encode() + b": ") and message in err, err


def test_allocation_seed_and_latent():
    c = MlaLatentCache(2, 100, BF16, "cpu")
    assert (c.k_img.shape, c.v_img.shape, c.k_scale.shape, c.v_scale.shape) == ((2, 2, 36864), (2, 2, 32768), (2, 8), (2, 512))
    assert (c.k_mean.shape, c.k_mean.dtype, c.v_amax.shape, c.v_amax.dtype) == ((2, 576), BF16, (2, 512), torch.float32)
    assert c.tail.shape == (2, 64, 576) and c.tail.dtype == BF16 and c.lens.dtype == torch.int32 and c.lens.tolist() == [0, 0]
    for unseeded in (c.latent, lambda: c.append(torch.zeros(2, 1, 576, dtype=BF16))):
        with pytest.raises(ValueError, match="no statistics"):
            unseeded()
    for k_mean, v_amax, match in ((torch.zeros(2, 576), torch.ones(2, 512), "k_mean"), (torch.zeros(2, 512, dtype=BF16), torch.ones(2, 512), "k_mean"),
                                  (None, torch.ones(2, 576), "v_amax"), (None, torch.ones(2, 512, dtype=torch.int32), "v_amax")):
        with pytest.raises(ValueError, match=match):
            c.seed(k_mean, v_amax)
    c.lens.fill_(7)
    km = torch.full((2, 576), 0.5, dtype=BF16)
    assert c.seed(km, torch.full((2, 512), 3.0, dtype=torch.float64)) is c
    lat = c.latent()
    assert c.lens.tolist() == [0, 0] and torch.equal(c.k_mean, km) and bool((c.v_amax == 3.0).all())
    assert lat is c.latent() and lat.kv_lens is c.lens and lat.Lk == 100 and lat.smooth_k
    assert all(getattr(lat, n) is getattr(c, n) for n in ("k_img", "v_img", "k_scale", "v_scale", "k_mean"))
    plain = MlaLatentCache(2, 64, F16, "cpu", smooth_k=False).seed(km.half(), torch.ones(2, 512))
    assert not plain.latent().smooth_k and not plain.k_mean.any()
    for bad in (dict(B=0), dict(capacity=0), dict(capacity=1.5), dict(dtype=torch.float32)):
        with pytest.raises(ValueError, match="MlaLatentCache: "):
            MlaLatentCache(**{**dict(B=2, capacity=64, dtype=F16, device="cpu"), **bad})


def test_append_and_from_prefill_value_errors_before_any_work(monkeypatch):
    c = MlaLatentCache(2, 64, F16, "cpu").seed(None, torch.ones(2, 512))
    h = lambda *s, dt=F16: torch.zeros(*s, dtype=dt)
    for kv_new, kw, match in ((h(2, 576), {}, r"3-D \[B, T, 576\]"),
                              (h(2, 1, 128), {}, "call sageattention_amd.sageattn for head_dim <= 128"),
                              (h(2, 1, 192), {}, "sageattn_qk192"), (h(2, 1, 256), {}, "sageattn_hd256"),
                              (h(2, 1, 576, dt=BF16), {}, "cache's dtype"), (h(2, 1, 576).to("meta"), {}, "cache's device"),
                              (h(3, 1, 576), {}, "cache's batch 2"), (h(2, 0, 576), {}, "at least one row"),
                              (h(2, 1, 1152)[..., ::2], {}, "Last dim of kv_new must be contiguous"),
                              (h(2, 1, 576), dict(new_lens=torch.zeros(2, dtype=torch.int64)), "new_lens must be a contiguous int32"),
                              (h(2, 1, 576), dict(new_lens=torch.zeros(3, dtype=torch.int32)), "new_lens"),
                              (h(2, 1, 576), dict(new_lens=[1, 1]), "new_lens")):
        with pytest.raises(ValueError, match=match):
            c.append(kv_new, **kw)
    assert c.lens.tolist() == [0, 0]
    for kv, match in ((h(2, 8, 576), "needs kv on a CUDA"), (h(2, 8, 512), "from_prefill takes latent rows of 576 channels")):
        with pytest.raises(ValueError, match=match):
            MlaLatentCache.from_prefill(kv)
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    for call, name in ((lambda: c.append(h(2, 1, 576)), "append"), (lambda: MlaLatentCache.from_prefill(h(2, 8, 576)), "from_prefill")):
        with pytest.raises(ValueError, match=f"MlaLatentCache.{name} is not supported under torch.compile"):
            call()
