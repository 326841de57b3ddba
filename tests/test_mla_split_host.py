"""CPU: the C boundary and Python interface of the exact split of the key range for the absorbed MLA decode call
(include/sage_mlasplit_gfx950.h, sageattention_amd/_cabi_mlasplit.py, ``sageattn_mla_decode(num_splits=)``).  The header's prototypes are the
binding's table; the entry refuses bad arguments with -1 and its message, in the header's order, before anything touches a GPU (host memory
only); bad ``num_splits`` values raise ValueError naming the keyword; the unsplit route's table and the package's public names did not move."""
import os
import re

import pytest
import torch

import util  # noqa: F401  (sys.path)
import test_paged_kv_host as paged
from test_kv_cache_host import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sage_mlasplit_gfx950.h")


def test_binding_is_the_header_and_nothing_else_moved():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, _cabi_mla, _cabi_mlasplit
    protos = _prototypes(HEADER, "SAGE_MLASPLIT_API")
    assert sorted(protos) == sorted(_cabi_mlasplit.SYMBOLS) == ["sage_mlasplit_abi_version", "sage_mlasplit_attn", "sage_mlasplit_ws_bytes"]
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_mlasplit.SYMBOLS[name]
        assert res is paged._ctype(ret) and [paged._ctype(c) for c in params] == list(argtypes), name
    # sage_mla_attn's arguments followed by num_splits, ws, ws_bytes
    assert list(_cabi_mlasplit.SYMBOLS["sage_mlasplit_attn"][1][:20]) == list(_cabi_mla.SYMBOLS["sage_mla_attn"][1])
    lib = _cabi_mlasplit.load()
    assert lib is _cabi.load() and lib.sage_mlasplit_abi_version() == _cabi_mlasplit.ABI_VERSION == 1
    assert sorted(_cabi_mla.SYMBOLS) == ["sage_mla_abi_version", "sage_mla_attn", "sage_mla_prepass", "sage_mla_ws_floats"]
    assert not any(n.startswith("sage_mla") for n in _cabi.SYMBOLS) and not any("mla" in n for n in sa.__all__)
    mk = open(os.path.join(ROOT, "sageattention_amd", "csrc", "Makefile")).read()
    assert "sage_mla_split.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert "../../include/sage_mlasplit_gfx950.h" in re.search(r"^HDRS\s*:=\s*(.*)$", mk, re.M).group(1).split()


@pytest.mark.parametrize("B,Lq,Hq,S", [(1, 1, 1, 2), (2, 3, 48, 5), (32, 2, 128, 255)])
def test_ws_bytes_is_three_segments_rounded_to_128(B, Lq, Hq, S):
    from sageattention_amd import _cabi_mlasplit
    lib, n = _cabi_mlasplit.load(), B * S * Lq * Hq
    assert lib.sage_mlasplit_ws_bytes(B, Lq, Hq, S) == 2 * ((4 * n + 127) // 128 * 128) + (2048 * n + 127) // 128 * 128
    for bad in ((0, Lq, Hq, S), (B, Lq, Hq, 1), (B, Lq, Hq, 256)):
        assert lib.sage_mlasplit_ws_bytes(*bad) == -1 and lib.sage_last_error().startswith(b"sage_mlasplit_ws_bytes: empty problem or num_splits")


def _args(p, **kw):
    a = dict(q=p, k_image=p, v_image=p, k_scale=p, v_scale=p, kv_lens=None, o=p, lse=None, B=1, Lq=1, Hq=2, Lk=1, width_qk=576, width_v=512,
             q_sb=1152, q_sl=1152, q_sh=576, sm_scale=1.0, dtype=1, stream=None, num_splits=2, ws=p, ws_bytes=2 * 128 + 8192)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("bad,message", [                       # the header's order: each case is good in everything in front of it
    (dict(width_qk=256, width_v=256, num_splits=1), b"width_qk must be 576 and width_v 512 (got 256 and 256)"),
    (dict(dtype=-1, num_splits=1), b"dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got -1)"),
    (dict(Lq=0, num_splits=1), b"empty problem (B 1, Lq 0, Hq 2, Lk 1)"),
    (dict(o=None, num_splits=1), b"null pointer (only kv_lens and lse may be null)"),
    (dict(q_sh=580, num_splits=1), b"q and o must be 16-byte aligned"),
    (dict(v_scale="+4", num_splits=1), b"the images and v_scale must be 16-byte aligned"),
    (dict(num_splits=1, ws=None), b"num_splits must be in [2, 255] (got 1); call sage_mla_attn"),
    (dict(num_splits=256, ws=None), b"num_splits must be in [2, 255] (got 256)"),
    (dict(ws=None, B=1 << 24, Hq=128), b"ws must be 128-byte aligned and hold sage_mlasplit_ws_bytes(B, Lq, Hq, num_splits) = "),
    (dict(ws="+64"), b"ws must be 128-byte aligned"),
    (dict(ws_bytes=8447), b"num_splits) = 8448 bytes (got 8447)"),
    (dict(B=1 << 24, Hq=128, num_splits=128, ws_bytes=1 << 62), b"B * ceil(Lq * Hq / 128) * num_splits and B * Lq * Hq / 4 must be below 2^31"),
])
def test_the_entry_refuses_with_its_message(bad, message):
    from sageattention_amd import _cabi_mlasplit
    lib = _cabi_mlasplit.load()
    buf, p = paged._aligned_buffer()
    p = (p + 127) // 128 * 128
    bad = {n: (p + int(x) if isinstance(x, str) else x) for n, x in bad.items()}       # "+n": the aligned address plus n bytes
    assert lib.sage_mlasplit_attn(*_args(p, **bad)) == -1
    err = lib.sage_last_error()
    assert err.startswith(b"sage_mlasplit_attn: ") and message in err, err


@pytest.mark.parametrize("B,rows,Lk,S", [(1, 128, 32768, 32), (8, 256, 8192, 16), (32, 128, 4096, 8), (128, 128, 8192, 2), (128, 256, 8192, 1),
                                         (32, 128, 4095, 1)])
def test_the_auto_plan_splits_only_where_the_probe_measured_a_gain(B, rows, Lk, S):
    from sageattention_amd.mla_decode import _auto_num_splits
    assert _auto_num_splits(B, rows, Lk) == S


@pytest.mark.parametrize("value", [256, -1, "eight", True, 2.0, [4]])
def test_bad_num_splits_is_a_value_error_that_names_the_keyword(value, monkeypatch):
    from sageattention_amd.mla_decode import sageattn_mla_decode
    q, kv = torch.zeros(1, 1, 2, 576, dtype=torch.float16), torch.zeros(1, 8, 576, dtype=torch.float16)
    with pytest.raises(ValueError, match="sageattn_mla_decode: num_splits must be None or 1"):
        sageattn_mla_decode(q, kv, num_splits=value)
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    with pytest.raises(ValueError, match="num_splits is not supported under torch.compile"):
        sageattn_mla_decode(q, kv, num_splits=4)
