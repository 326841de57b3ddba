"""CPU: the head_dim = 256 route's C boundary and Python interface (include/sage_hd256_gfx950.h, sageattention_amd/_cabi_hd256.py,
sageattention_amd/hd256.py).  The header's prototypes are the binding's table; the two entries refuse bad arguments with -1 and their message
before anything touches a GPU (host memory only); the Python function raises ValueError; the package's public names did not move."""
import ctypes
import os

import pytest
import torch

import util  # noqa: F401  (sys.path)
import test_paged_kv_host as paged
from test_kv_cache_host import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sage_hd256_gfx950.h")


def test_binding_is_the_header_and_the_package_names_stay():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, _cabi_hd256
    protos = _prototypes(HEADER, "SAGE_HD256_API")
    assert sorted(protos) == sorted(_cabi_hd256.SYMBOLS) == ["sage_hd256_abi_version", "sage_hd256_attn", "sage_hd256_prepass", "sage_hd256_ws_floats"]
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_hd256.SYMBOLS[name]
        assert res is paged._ctype(ret) and [paged._ctype(c) for c in params] == list(argtypes), name
    assert _cabi_hd256.load() is _cabi.load() and _cabi_hd256.load().sage_hd256_abi_version() == _cabi_hd256.ABI_VERSION == 1
    assert not any(n.startswith("sage_hd256") for n in _cabi.SYMBOLS) and "sageattn_hd256" not in sa.__all__


def _args(p, entry, **kw):
    if entry == "sage_hd256_prepass":
        a = dict(k=p, v=p, k_image=p, k_scale=p, k_mean=p, v_image=p, v_scale=p, ws=p, ws_floats=512, B=1, Hkv=1, Lk=1, head_dim=256,
                 k_sb=256, k_sh=256, k_sl=256, v_sb=256, v_sh=256, v_sl=256, smooth_k=1, dtype=0, stream=None)
    else:
        a = dict(q=p, k_image=p, v_image=p, k_scale=p, v_scale=p, o=p, lse=None, B=1, Hq=2, Hkv=1, Lq=1, Lk=1, head_dim=256,
                 q_sb=512, q_sh=256, q_sl=256, o_sb=512, o_sh=256, o_sl=256, is_causal=0, sm_scale=1.0, dtype=1, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("entry,bad,message", [
    ("sage_hd256_prepass", dict(head_dim=128), b"head_dim must be 256 (got 128)"),
    ("sage_hd256_prepass", dict(dtype=2), b"dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got 2)"),
    ("sage_hd256_prepass", dict(Lk=0), b"empty problem (B 1, Hkv 1, Lk 0)"),
    ("sage_hd256_prepass", dict(k_mean=None), b"null pointer"),
    ("sage_hd256_prepass", dict(k="+2"), b"k and v must be 16-byte aligned"),
    ("sage_hd256_prepass", dict(v_sl=252), b"k and v must be 16-byte aligned"),
    ("sage_hd256_prepass", dict(ws_floats=511), b"ws holds 511 floats, sage_hd256_ws_floats(B, Hkv, Lk) = 512"),
    ("sage_hd256_attn", dict(head_dim=192), b"head_dim must be 256 (got 192)"),
    ("sage_hd256_attn", dict(dtype=-1), b"dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got -1)"),
    ("sage_hd256_attn", dict(Lq=0), b"empty problem (B 1, Hq 2, Hkv 1, Lq 0, Lk 1)"),
    ("sage_hd256_attn", dict(Hq=3, Hkv=2), b"Hq (3) must be a multiple of Hkv (2)"),
    ("sage_hd256_attn", dict(o=None), b"null pointer (only lse may be null)"),
    ("sage_hd256_attn", dict(q="+8"), b"q and o must be 16-byte aligned"),
    ("sage_hd256_attn", dict(v_scale="+4"), b"the images and v_scale must be 16-byte aligned"),
])
def test_the_c_entries_refuse_with_their_message(entry, bad, message):
    from sageattention_amd import _cabi_hd256
    lib = _cabi_hd256.load()
    buf, p = paged._aligned_buffer()
    bad = {n: (p + int(x) if isinstance(x, str) else x) for n, x in bad.items()}       # "+n": the aligned address plus n bytes
    assert getattr(lib, entry)(*_args(p, entry, **bad)) == -1
    err = lib.sage_last_error()
    assert err.startswith(entry.encode() + b": ") and message in err, err


@pytest.mark.parametrize("shape,dtype,message", [
    ((1, 2, 8, 128), torch.float16, "call sageattention_amd.sageattn"),
    ((1, 2, 8, 64), torch.bfloat16, "call sageattention_amd.sageattn"),
    ((1, 2, 8, 264), torch.float16, "Unsupported head_dim: 264"),
    ((1, 2, 8, 256), torch.float16, "CUDA (ROCm) device"),
    ((1, 2, 8, 256), torch.float32, "CUDA (ROCm) device"),
])
def test_the_python_function_refuses_with_value_error(shape, dtype, message):
    from sageattention_amd.hd256 import sageattn_hd256
    x = torch.zeros(shape, dtype=dtype)
    with pytest.raises(ValueError, match=message.replace("(", r"\(").replace(")", r"\)")):
        sageattn_hd256(x, x, x)
