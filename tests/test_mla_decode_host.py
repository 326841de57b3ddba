"""CPU: the C boundary and Python interface of the absorbed MLA decode route (include/sage_mla_gfx950.h, sageattention_amd/_cabi_mla.py,
sageattention_amd/mla_decode.py).  The header's prototypes are the binding's table; the entries refuse bad arguments with -1 and their message
before anything touches a GPU (host memory only); the Python functions raise ValueError and name the entry to call instead; the package's public
names did not move."""
import os

import pytest
import torch

import util  # noqa: F401  (sys.path)
import test_paged_kv_host as paged
from test_kv_cache_host import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sage_mla_gfx950.h")


def test_binding_is_the_header_and_the_package_names_stay():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, _cabi_mla
    protos = _prototypes(HEADER, "SAGE_MLA_API")
    assert sorted(protos) == sorted(_cabi_mla.SYMBOLS) == ["sage_mla_abi_version", "sage_mla_attn", "sage_mla_prepass", "sage_mla_ws_floats"]
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_mla.SYMBOLS[name]
        assert res is paged._ctype(ret) and [paged._ctype(c) for c in params] == list(argtypes), name
    lib = _cabi_mla.load()
    assert lib is _cabi.load() and lib.sage_mla_abi_version() == _cabi_mla.ABI_VERSION == 1
    assert not any(n.startswith("sage_mla") for n in _cabi.SYMBOLS) and "sageattn_mla_decode" not in sa.__all__
    # 1088 floats per (sample, 256-token chunk) and 512 more per sample
    assert lib.sage_mla_ws_floats(1, 1) == 1600 and lib.sage_mla_ws_floats(3, 257) == 3 * (2 * 1088 + 512)
    assert lib.sage_mla_ws_floats(0, 5) == -1 and b"sage_mla_ws_floats: empty problem (B 0, Lk 5)" in lib.sage_last_error()


def _args(p, entry, **kw):
    if entry == "sage_mla_prepass":
        a = dict(kv=p, kv_lens=None, k_image=p, k_scale=p, k_mean=p, v_image=p, v_scale=p, ws=p, ws_floats=1600, B=1, Lk=1, width_qk=576,
                 width_v=512, kv_sb=576, kv_sl=576, smooth_k=1, dtype=0, stream=None)
    else:
        a = dict(q=p, k_image=p, v_image=p, k_scale=p, v_scale=p, kv_lens=None, o=p, lse=None, B=1, Lq=1, Hq=2, Lk=1, width_qk=576, width_v=512,
                 q_sb=1152, q_sl=1152, q_sh=576, sm_scale=1.0, dtype=1, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("entry,bad,message", [
    ("sage_mla_prepass", dict(width_qk=192, width_v=128), b"width_qk must be 576 and width_v 512 (got 192 and 128); call sage_qk192_prepass"),
    ("sage_mla_prepass", dict(width_v=576), b"width_qk must be 576 and width_v 512 (got 576 and 576)"),
    ("sage_mla_prepass", dict(dtype=2), b"dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got 2)"),
    ("sage_mla_prepass", dict(Lk=0), b"empty problem (B 1, Lk 0)"),
    ("sage_mla_prepass", dict(k_mean=None), b"null pointer (only kv_lens may be null)"),
    ("sage_mla_prepass", dict(kv="+2"), b"kv must be 16-byte aligned"),
    ("sage_mla_prepass", dict(kv_sl=568), b"a token stride of at least 576"),
    ("sage_mla_prepass", dict(kv_lens="+2"), b"ws and kv_lens 4-byte"),
    ("sage_mla_prepass", dict(ws_floats=1599), b"ws holds 1599 floats, sage_mla_ws_floats(B, Lk) = 1600"),
    ("sage_mla_prepass", dict(B=65536, ws_floats=1 << 40), b"B must be at most 65535 (got 65536)"),
    ("sage_mla_attn", dict(width_qk=256, width_v=256), b"width_qk must be 576 and width_v 512 (got 256 and 256); call sage_qk192_attn"),
    ("sage_mla_attn", dict(dtype=-1), b"dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got -1)"),
    ("sage_mla_attn", dict(Lq=0), b"empty problem (B 1, Lq 0, Hq 2, Lk 1)"),
    ("sage_mla_attn", dict(o=None), b"null pointer (only kv_lens and lse may be null)"),
    ("sage_mla_attn", dict(q="+8"), b"q and o must be 16-byte aligned"),
    ("sage_mla_attn", dict(q_sh=580), b"q and o must be 16-byte aligned"),
    ("sage_mla_attn", dict(v_scale="+4"), b"the images and v_scale must be 16-byte aligned"),
])
def test_the_c_entries_refuse_with_their_message(entry, bad, message):
    from sageattention_amd import _cabi_mla
    lib = _cabi_mla.load()
    buf, p = paged._aligned_buffer()
    bad = {n: (p + int(x) if isinstance(x, str) else x) for n, x in bad.items()}       # "+n": the aligned address plus n bytes
    assert getattr(lib, entry)(*_args(p, entry, **bad)) == -1
    err = lib.sage_last_error()
    assert err.startswith(entry.encode() + b": ") and message in err, err


@pytest.mark.parametrize("kv_shape,dtype,lens,message", [
    ((1, 8, 128), torch.float16, None, "call sageattention_amd.sageattn for"),
    ((1, 8, 192), torch.bfloat16, None, "call sageattention_amd.qk192.sageattn_qk192"),
    ((1, 8, 256), torch.float16, None, "call sageattention_amd.hd256.sageattn_hd256"),
    ((1, 1, 8, 576), torch.float16, None, "kv must be 3-D"),
    ((1, 8, 576), torch.float32, None, "kv must be torch.float16 or torch.bfloat16"),
    ((2, 8, 576), torch.float16, torch.zeros(2, dtype=torch.int64), "kv_lens must be an int32 tensor of shape [2]"),
    ((2, 8, 576), torch.float16, torch.zeros(3, dtype=torch.int32), "kv_lens must be an int32 tensor of shape [2]"),
    ((1, 8, 576), torch.float16, None, "CUDA (ROCm) device"),
])
def test_the_python_functions_refuse_with_value_error(kv_shape, dtype, lens, message):
    from sageattention_amd.mla_decode import mla_quantize_latent, sageattn_mla_decode
    kv, q = torch.zeros(kv_shape, dtype=dtype), torch.zeros((kv_shape[0], 1, 2, 576), dtype=dtype)
    pattern = message.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")
    with pytest.raises(ValueError, match=pattern):
        mla_quantize_latent(kv, lens)
    with pytest.raises(ValueError, match=pattern):
        sageattn_mla_decode(q, kv, lens)


def test_refused_under_torch_compile(monkeypatch):
    from sageattention_amd.mla_decode import sageattn_mla_decode
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    with pytest.raises(ValueError, match="not supported under torch.compile"):
        sageattn_mla_decode(torch.zeros(1, 1, 2, 576), torch.zeros(1, 8, 576))
