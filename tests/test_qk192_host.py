"""CPU: the C boundary and Python interface of the 192-wide Q / K, 128-wide V route (include/sage_qk192_gfx950.h,
sageattention_amd/_cabi_qk192.py, sageattention_amd/qk192.py).  The header's prototypes are the binding's table; the two entries refuse bad
arguments with -1 and their message before anything touches a GPU (host memory only); the Python function raises ValueError and names the entry
to call instead; the package's public names did not move."""
import os

import pytest
import torch

import util  # noqa: F401  (sys.path)
import test_paged_kv_host as paged
from test_kv_cache_host import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sage_qk192_gfx950.h")


def test_binding_is_the_header_and_the_package_names_stay():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, _cabi_qk192
    protos = _prototypes(HEADER, "SAGE_QK192_API")
    assert sorted(protos) == sorted(_cabi_qk192.SYMBOLS) == ["sage_qk192_abi_version", "sage_qk192_attn", "sage_qk192_prepass", "sage_qk192_ws_floats"]
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_qk192.SYMBOLS[name]
        assert res is paged._ctype(ret) and [paged._ctype(c) for c in params] == list(argtypes), name
    assert _cabi_qk192.load() is _cabi.load() and _cabi_qk192.load().sage_qk192_abi_version() == _cabi_qk192.ABI_VERSION == 1
    assert not any(n.startswith("sage_qk192") for n in _cabi.SYMBOLS) and "sageattn_qk192" not in sa.__all__


def _args(p, entry, **kw):
    if entry == "sage_qk192_prepass":
        a = dict(k=p, v=p, k_image=p, k_scale=p, k_mean=p, v_image=p, v_scale=p, ws=p, ws_floats=320, B=1, Hkv=1, Lk=1, head_dim_qk=192,
                 head_dim_v=128, k_sb=192, k_sh=192, k_sl=192, v_sb=128, v_sh=128, v_sl=128, smooth_k=1, dtype=0, stream=None)
    else:
        a = dict(q=p, k_image=p, v_image=p, k_scale=p, v_scale=p, o=p, lse=None, B=1, Hq=2, Hkv=1, Lq=1, Lk=1, head_dim_qk=192, head_dim_v=128,
                 q_sb=384, q_sh=192, q_sl=192, o_sb=256, o_sh=128, o_sl=128, is_causal=0, sm_scale=1.0, dtype=1, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("entry,bad,message", [
    ("sage_qk192_prepass", dict(head_dim_qk=256), b"head_dim_qk must be 192 and head_dim_v 128 (got 256 and 128)"),
    ("sage_qk192_prepass", dict(head_dim_v=192), b"head_dim_qk must be 192 and head_dim_v 128 (got 192 and 192)"),
    ("sage_qk192_prepass", dict(dtype=2), b"dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got 2)"),
    ("sage_qk192_prepass", dict(Lk=0), b"empty problem (B 1, Hkv 1, Lk 0)"),
    ("sage_qk192_prepass", dict(k_mean=None), b"null pointer"),
    ("sage_qk192_prepass", dict(k="+2"), b"k and v must be 16-byte aligned"),
    ("sage_qk192_prepass", dict(k_sl=184), b"k and v must be 16-byte aligned"),
    ("sage_qk192_prepass", dict(v_sl=120), b"k and v must be 16-byte aligned"),
    ("sage_qk192_prepass", dict(ws_floats=319), b"ws holds 319 floats, sage_qk192_ws_floats(B, Hkv, Lk) = 320"),
    ("sage_qk192_attn", dict(head_dim_qk=128), b"head_dim_qk must be 192 and head_dim_v 128 (got 128 and 128)"),
    ("sage_qk192_attn", dict(head_dim_v=64), b"head_dim_qk must be 192 and head_dim_v 128 (got 192 and 64)"),
    ("sage_qk192_attn", dict(dtype=-1), b"dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got -1)"),
    ("sage_qk192_attn", dict(Lq=0), b"empty problem (B 1, Hq 2, Hkv 1, Lq 0, Lk 1)"),
    ("sage_qk192_attn", dict(Hq=3, Hkv=2), b"Hq (3) must be a multiple of Hkv (2)"),
    ("sage_qk192_attn", dict(o=None), b"null pointer (only lse may be null)"),
    ("sage_qk192_attn", dict(q="+8"), b"q and o must be 16-byte aligned"),
    ("sage_qk192_attn", dict(o_sl=120), b"q and o must be 16-byte aligned"),
    ("sage_qk192_attn", dict(v_scale="+4"), b"the images and v_scale must be 16-byte aligned"),
])
def test_the_c_entries_refuse_with_their_message(entry, bad, message):
    from sageattention_amd import _cabi_qk192
    lib = _cabi_qk192.load()
    buf, p = paged._aligned_buffer()
    bad = {n: (p + int(x) if isinstance(x, str) else x) for n, x in bad.items()}       # "+n": the aligned address plus n bytes
    assert getattr(lib, entry)(*_args(p, entry, **bad)) == -1
    err = lib.sage_last_error()
    assert err.startswith(entry.encode() + b": ") and message in err, err


@pytest.mark.parametrize("dqk,dv,dtype,message", [
    (128, 128, torch.float16, "call sageattention_amd.sageattn for"),
    (200, 128, torch.bfloat16, "call sageattention_amd.hd256.sageattn_hd256 with v zero-padded"),
    (192, 136, torch.float16, "call sageattention_amd.hd256.sageattn_hd256 with v zero-padded"),
    (264, 128, torch.float16, "Unsupported head_dim: 264"),
    (192, 128, torch.float16, "CUDA (ROCm) device"),
])
def test_the_python_function_refuses_with_value_error(dqk, dv, dtype, message):
    from sageattention_amd.qk192 import sageattn_qk192
    qk, v = torch.zeros((1, 2, 8, dqk), dtype=dtype), torch.zeros((1, 2, 8, dv), dtype=dtype)
    with pytest.raises(ValueError, match=message.replace("(", r"\(").replace(")", r"\)")):
        sageattn_qk192(qk, qk, v)
