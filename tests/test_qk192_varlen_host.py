"""CPU: the C boundary and Python interface of the packed 192-wide Q / K, 128-wide V route (include/sage_qk192v_gfx950.h,
sageattention_amd/_cabi_qk192v.py, sageattention_amd/qk192_varlen.py).  The header's prototypes are the binding's table; the two entries refuse
bad arguments with -1 and their message before anything touches a GPU (host memory only); the Python function raises ValueError and names the
entry to call instead; the host-side size bounds hold for the sequence lists of tests/test_gpu_qk192_varlen.py."""
import os

import pytest
import torch

import util  # noqa: F401  (sys.path)
import test_paged_kv_host as paged
from test_kv_cache_host import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sage_qk192v_gfx950.h")
# the sequence lists of the GPU test: (Lq_s, Lk_s)
LISTS = [
    [(1, 1)],
    [(33, 65), (128, 64), (1, 200)],
    [(129, 192), (0, 70), (257, 449)],
    [(72, 200), (40, 0), (200, 72)],
    [(130, 450), (64, 64)],
]


def test_binding_is_the_header_and_the_package_names_stay():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, _cabi_qk192, _cabi_qk192v
    protos = _prototypes(HEADER, "SAGE_QK192V_API")
    assert sorted(protos) == sorted(_cabi_qk192v.SYMBOLS) == ["sage_qk192v_abi_version", "sage_qk192v_attn", "sage_qk192v_prepass", "sage_qk192v_ws_bytes"]
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_qk192v.SYMBOLS[name]
        assert res is paged._ctype(ret) and [paged._ctype(c) for c in params] == list(argtypes), name
    assert _cabi_qk192v.load() is _cabi.load() and _cabi_qk192v.load().sage_qk192v_abi_version() == _cabi_qk192v.ABI_VERSION == 1
    assert not any(n.startswith("sage_qk192v") for n in list(_cabi.SYMBOLS) + list(_cabi_qk192.SYMBOLS)) and "sageattn_qk192_varlen" not in sa.__all__


def _args(p, entry, **kw):
    if entry == "sage_qk192v_prepass":
        a = dict(k=p, v=p, cu_seqlens_q=p, cu_seqlens_k=p, k_image=p, k_scale=p, k_mean=p, v_image=p, v_scale=p, ws=p, ws_bytes=1 << 20, nseq=2,
                 total_q=8, total_k=8, Hq=2, Hkv=1, head_dim_qk=192, head_dim_v=128, k_sl=192, k_sh=192, v_sl=128, v_sh=128, mask=2, smooth_k=1,
                 dtype=0, stream=None)
    else:
        a = dict(q=p, cu_seqlens_q=p, cu_seqlens_k=p, k_image=p, v_image=p, k_scale=p, v_scale=p, ws=p, ws_bytes=1 << 20, o=p, lse=None, nseq=2,
                 total_q=8, total_k=8, Hq=2, Hkv=1, head_dim_qk=192, head_dim_v=128, q_sl=384, q_sh=192, o_sl=256, o_sh=128, mask=0, sm_scale=1.0,
                 dtype=1, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("entry,bad,message", [
    ("sage_qk192v_prepass", dict(head_dim_qk=128), b"head_dim_qk must be 192 and head_dim_v 128 (got 128 and 128)"),
    ("sage_qk192v_prepass", dict(dtype=2), b"dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got 2)"),
    ("sage_qk192v_prepass", dict(mask=3), b"mask must be 0 (none), 1 (causal top-left) or 2 (causal bottom-right) (got 3)"),
    ("sage_qk192v_prepass", dict(total_k=0), b"empty problem (Hq 2, Hkv 1, total_q 8, total_k 0)"),
    ("sage_qk192v_prepass", dict(nseq=1025), b"nseq must be in 1 .. 1024 (got 1025)"),
    ("sage_qk192v_prepass", dict(Hq=3, Hkv=2), b"Hq (3) must be a multiple of Hkv (2)"),
    ("sage_qk192v_prepass", dict(cu_seqlens_k=None), b"null pointer"),
    ("sage_qk192v_prepass", dict(k="+2"), b"k and v must be 16-byte aligned"),
    ("sage_qk192v_prepass", dict(k_sh=184), b"k and v must be 16-byte aligned"),
    ("sage_qk192v_prepass", dict(ws="+4"), b"the images and ws must be 16-byte aligned"),
    ("sage_qk192v_prepass", dict(ws_bytes=64), b"ws holds 64 bytes, sage_qk192v_ws_bytes(nseq, Hkv, total_q, total_k) = "),
    ("sage_qk192v_attn", dict(head_dim_v=64), b"head_dim_qk must be 192 and head_dim_v 128 (got 192 and 64)"),
    ("sage_qk192v_attn", dict(dtype=-1), b"dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got -1)"),
    ("sage_qk192v_attn", dict(mask=-1), b"mask must be 0 (none), 1 (causal top-left) or 2 (causal bottom-right) (got -1)"),
    ("sage_qk192v_attn", dict(total_q=0), b"empty problem (Hq 2, Hkv 1, total_q 0, total_k 8)"),
    ("sage_qk192v_attn", dict(nseq=0), b"nseq must be in 1 .. 1024 (got 0)"),
    ("sage_qk192v_attn", dict(o=None), b"null pointer (only lse may be null)"),
    ("sage_qk192v_attn", dict(o_sh=120), b"q and o must be 16-byte aligned"),
    ("sage_qk192v_attn", dict(v_scale="+4"), b"the images, v_scale and ws must be 16-byte aligned"),
    ("sage_qk192v_attn", dict(ws_bytes=0), b"ws holds 0 bytes"),
])
def test_the_c_entries_refuse_with_their_message(entry, bad, message):
    from sageattention_amd import _cabi_qk192v
    lib = _cabi_qk192v.load()
    buf, p = paged._aligned_buffer()
    bad = {n: (p + int(x) if isinstance(x, str) else x) for n, x in bad.items()}       # "+n": the aligned address plus n bytes
    assert getattr(lib, entry)(*_args(p, entry, **bad)) == -1
    err = lib.sage_last_error()
    assert err.startswith(entry.encode() + b": ") and message in err, err


@pytest.mark.parametrize("shape,kw,message", [
    ((128, 128), dict(is_causal=True), "call sageattention_amd.sageattn_qk_int8_pv_fp8_varlen for"),
    ((200, 128), dict(is_causal=True), "no packed route is wider"),
    ((192, 136), dict(causal_align="top_left"), "no packed route is wider"),
    ((192, 128), dict(is_causal=False, causal_align="bottom_right"), 'causal_align="bottom_right" needs is_causal=True'),
    ((192, 128), dict(is_causal=True, causal_align="middle"), 'causal_align must be "top_left" or "bottom_right"'),
    ((192, 128), dict(is_causal=True), "CUDA (ROCm) device"),
    ((192, 128), dict(is_causal=True, dtype=torch.float32), "CUDA (ROCm) device"),
])
def test_the_python_function_refuses_with_value_error(shape, kw, message):
    from sageattention_amd.qk192_varlen import sageattn_qk192_varlen
    dtype = kw.pop("dtype", torch.float16)
    qk, v = torch.zeros((8, 2, shape[0]), dtype=dtype), torch.zeros((8, 2, shape[1]), dtype=dtype)
    cu = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(ValueError, match=message.replace("(", r"\(").replace(")", r"\)")):
        sageattn_qk192_varlen(qk, qk, v, cu, cu, 8, 8, **kw)


@pytest.mark.parametrize("seqs", LISTS)
def test_the_host_size_bounds_hold(seqs):
    """The buffers and grids are sized without the lengths: ceil(total_q / 128) + nseq items, ceil(total_k / 64) + nseq tiles, and the workspace
    query's plan holds them."""
    from sageattention_amd import _cabi_qk192v
    from sageattention_amd.qk192_varlen import size_bounds
    total_q, total_k, nseq = sum(a for a, _ in seqs), sum(b for _, b in seqs), len(seqs)
    items, tiles, chunks = size_bounds(max(total_q, 1), max(total_k, 1), nseq)
    assert sum((a + 127) // 128 for a, _ in seqs) <= items == (total_q + 127) // 128 + nseq
    assert sum((b + 63) // 64 for _, b in seqs) <= tiles == (total_k + 63) // 64 + nseq
    assert sum((b + 255) // 256 for _, b in seqs) <= chunks
    plan_ints = 16 + 2 * (nseq + 1) + 2 * items + tiles + chunks
    assert _cabi_qk192v.load().sage_qk192v_ws_bytes(nseq, 2, total_q, total_k) == 4 * ((plan_ints + 3) // 4 * 4 + 2 * chunks * 320)
