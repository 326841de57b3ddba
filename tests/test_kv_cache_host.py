"""CPU: the appendable KV cache's C boundary and Python interface (include/sage_kvcache_gfx950.h, sageattention_amd/_cabi_kvcache.py,
sageattention_amd/kv_cache.py).  The new header's prototypes are the new binding's table, the library exports them, every argument error
returns -1 with its message before anything touches a GPU, the Python layer raises ValueError before any work -- and none of it moved what the
main header, its binding and the package's ``__all__`` pin."""
import ctypes
import os
import re

import pytest
import torch

import util  # noqa: F401  (sys.path)
import sageattention_amd as sa
from sageattention_amd import _cabi, _cabi_kvcache
from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sage_kvcache_gfx950.h")
MAIN_HEADER = os.path.join(ROOT, "include", "sage_gfx950.h")


def _text(path):
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def _prototypes(path, macro):
    """name -> (return type, [parameter type, ...]) of every `macro` prototype of a header, types as written"""
    out = {}
    for ret, name, args in re.findall(macro + r"\s+([\w\s\*]+?)\b(sage_\w+)\s*\(([^)]*)\)\s*;", _text(path)):
        params = []
        for a in ([] if args.strip() == "void" else args.split(",")):
            ctype, _ = re.fullmatch(r"\s*(.*?)(\w+)\s*", a, flags=re.S).groups()
            params.append(" ".join(ctype.split()))
        assert name not in out, f"{name} declared twice"
        out[name] = (" ".join(ret.split()), params)
    return out


def _ctype_of(ctype):
    if ctype == "const char *":
        return ctypes.c_char_p
    if ctype.endswith("*"):
        return ctypes.c_void_p
    return {"void": None, "int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[ctype]


def test_binding_is_the_header():
    protos = _prototypes(HEADER, "SAGE_KVCACHE_API")
    assert sorted(protos) == sorted(_cabi_kvcache.SYMBOLS) == ["sage_kvcache_abi_version", "sage_kvcache_append"]
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_kvcache.SYMBOLS[name]
        assert res is _ctype_of(ret), f"{name}: returns {ret}, bound as {res}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters declared, {len(argtypes)} bound"
        for i, (ctype, bound) in enumerate(zip(params, argtypes)):
            assert bound is _ctype_of(ctype), f"{name}: parameter {i} ({ctype}) bound as {bound}"
    version = int(re.search(r"#define\s+SAGE_KVCACHE_ABI_VERSION\s+(\d+)", _text(HEADER)).group(1))
    assert version == 1 == _cabi_kvcache.ABI_VERSION
    assert "SAGE_API" not in re.sub(r"SAGE_KVCACHE_API", "", _text(HEADER))         # an export macro of its own


def test_library_exports_the_entries():
    lib = ctypes.CDLL(_cabi.LIB_PATH)
    for name in _cabi_kvcache.SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
    assert _cabi_kvcache.load() is _cabi.load()                      # one library, bound behind _cabi.load()
    assert _cabi_kvcache.load().sage_kvcache_abi_version() == 1


def test_existing_boundary_did_not_move():
    """What the existing tests pin: ABI 22, 56 prototypes in the main header, 56 bound symbols, the package's __all__."""
    lib = _cabi.load()
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22
    assert len(_prototypes(MAIN_HEADER, "SAGE_API")) == 56 and len(_cabi.SYMBOLS) == 56
    assert not any(n.startswith("sage_kvcache") for n in _cabi.SYMBOLS)
    assert sorted(sa.__all__) == sorted(["sageattn", "sageattn_varlen", "sageattn_qk_int8_pv_fp16_triton", "sageattn_qk_int8_pv_fp16_cuda",
                                         "sageattn_qk_int8_pv_fp8_cuda", "sageattn_qk_int8_pv_fp8_cuda_sm90", "sageattn_qk_int8_pv_fp8_varlen"])
    assert not hasattr(sa, "sageattn_kvcache") or "sageattn_kvcache" not in sa.__all__


def _append(lib, p, **kw):
    a = dict(k_int8=p, k_scale=p, v_image=p, v_scale=p, v_amax=p, k_mean=None, k_tail=p, v_tail=p, lens=p, k_new=p, v_new=p, new_lens=None,
             B=1, Hkv=1, capacity=64, T=1, head_dim=64, k_sb=64, k_sh=64, k_sl=64, v_sb=64, v_sh=64, v_sl=64, dtype=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.sage_kvcache_append(*a.values()), lib.sage_last_error()


CACHE_POINTERS = ("k_int8", "k_scale", "v_image", "v_scale", "v_amax", "k_tail", "v_tail", "lens")


def test_argument_errors_do_not_need_a_gpu():
    """Every refusal comes before anything touches a GPU (this machine may have none); the message goes through sage_last_error()."""
    lib = _cabi_kvcache.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    for name in CACHE_POINTERS:
        rc, msg = _append(lib, p, **{name: None})
        assert rc == -1 and b"null cache pointer" in msg, (name, rc, msg)
    for name in ("k_new", "v_new"):
        rc, msg = _append(lib, p, **{name: None})
        assert rc == -1 and b"null k_new / v_new" in msg, (name, rc, msg)
    for D in (0, 32, 96, 256):
        rc, msg = _append(lib, p, head_dim=D)
        assert rc == -1 and b"head_dim must be 64 or 128" in msg
    for T in (0, -3):
        rc, msg = _append(lib, p, T=T)
        assert rc == -1 and b"T must be at least 1" in msg
    for cap in (0, -64, 63, 100):
        rc, msg = _append(lib, p, capacity=cap)
        assert rc == -1 and b"capacity must be a positive multiple of 64" in msg
    for name in ("k_int8", "k_scale", "v_image", "k_tail", "v_tail", "k_new", "v_new", "k_mean"):
        rc, msg = _append(lib, p, **{name: p + 2})
        assert rc == -1 and b"16-byte aligned" in msg, (name, rc, msg)
    for name in ("k_sb", "k_sh", "k_sl", "v_sb", "v_sh", "v_sl"):
        rc, msg = _append(lib, p, **{name: 68})
        assert rc == -1 and b"multiples of 8 elements" in msg, (name, rc, msg)
    rc, msg = _append(lib, p, dtype=2)
    assert rc == -1 and b"dtype" in msg
    rc, msg = _append(lib, p, B=0)
    assert rc == -1 and b"B and Hkv" in msg
    with pytest.raises(ValueError, match="B and Hkv"):
        _cabi.check(rc, "sage_kvcache_append")


def _cache(dtype=torch.float16, seeded=True):
    c = QuantizedKVCache.allocate(2, 2, 100, 64, dtype, "cpu")
    if seeded:
        c.seed(torch.zeros(2, 2, 64, dtype=dtype), torch.ones(2, 2, 64))
    return c


def test_allocate_shapes_and_errors():
    c = _cache(seeded=False)
    assert c.capacity == 128 and (c.B, c.Hkv, c.D, c.dtype) == (2, 2, 64, torch.float16)
    assert c.k_int8.shape == (2, 2, 128, 64) and c.k_int8.dtype == torch.int8
    assert c.k_scale.shape == (2, 2, 8) and c.k_scale.dtype == torch.float32
    assert c.v_image.shape == (2, 2, 2, 64, 64) and c.v_image.dtype == torch.uint8
    assert c.v_scale.shape == c.v_amax.shape == (2, 2, 64) and c.v_scale.dtype == c.v_amax.dtype == torch.float32
    assert c.k_mean.shape == (2, 2, 64) and c.k_mean.dtype == torch.float16
    assert c.k_tail.shape == c.v_tail.shape == (2, 2, 64, 64) and c.k_tail.dtype == torch.float16
    assert c.lens.shape == (2,) and c.lens.dtype == torch.int32 and c.lens.tolist() == [0, 0]
    assert all(t.is_contiguous() for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail, c.lens))
    for bad in (dict(D=96), dict(D=256), dict(B=0), dict(Hkv=0), dict(capacity=0), dict(dtype=torch.float32), dict(capacity=1.5)):
        kw = dict(B=2, Hkv=2, capacity=64, D=64, dtype=torch.float16, device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError):
            QuantizedKVCache.allocate(**kw)


def test_seed_errors_and_state():
    c = _cache(seeded=False)
    with pytest.raises(ValueError, match="k_mean"):
        c.seed(torch.zeros(2, 2, 64), torch.ones(2, 2, 64))                              # dtype
    with pytest.raises(ValueError, match="k_mean"):
        c.seed(torch.zeros(2, 2, 128, dtype=torch.float16), torch.ones(2, 2, 64))        # shape
    with pytest.raises(ValueError, match="v_amax"):
        c.seed(None, torch.ones(2, 64))
    with pytest.raises(ValueError, match="v_amax"):
        c.seed(None, torch.ones(2, 2, 64, dtype=torch.int32))
    c.lens.fill_(7)
    km = torch.full((2, 2, 64), 0.5, dtype=torch.float16)
    assert c.seed(km, torch.full((2, 2, 64), 3.0, dtype=torch.float64)) is c
    assert c.lens.tolist() == [0, 0] and torch.equal(c.k_mean, km) and c.v_amax.dtype == torch.float32 and bool((c.v_amax == 3.0).all())
    c.seed(None, torch.ones(2, 2, 64))
    assert c.k_mean is None
    c.seed(km, torch.ones(2, 2, 64))
    assert torch.equal(c.k_mean, km)


def test_append_value_errors_before_any_work():
    h = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt)
    with pytest.raises(ValueError, match="no statistics"):
        _cache(seeded=False).append(h(2, 2, 1, 64), h(2, 2, 1, 64))
    c = _cache()
    for k_new, v_new, kw, match in (
            (h(2, 2, 1, 64, dt=torch.bfloat16), h(2, 2, 1, 64, dt=torch.bfloat16), {}, "dtype"),
            (h(2, 2, 1, 64), h(2, 2, 1, 64, dt=torch.bfloat16), {}, "dtype"),
            (h(2, 2, 1, 64), h(2, 2, 2, 64), {}, "one shape"),
            (h(3, 2, 1, 64), h(3, 2, 1, 64), {}, "B, Hkv, D"),
            (h(2, 4, 1, 64), h(2, 4, 1, 64), {}, "B, Hkv, D"),
            (h(2, 2, 1, 128), h(2, 2, 1, 128), {}, "B, Hkv, D"),
            (h(2, 2, 1, 64), h(2, 2, 1, 64), dict(tensor_layout="NHD"), "B, Hkv, D"),         # read as [B, T, Hkv, D]: Hkv = 1
            (h(2, 2, 0, 64), h(2, 2, 0, 64), {}, "at least one row"),
            (h(2, 2, 64), h(2, 2, 64), {}, "4-D"),
            (h(2, 2, 1, 64), h(2, 2, 1, 64), dict(tensor_layout="HDN"), "layout"),
            (h(2, 2, 1, 64), h(2, 2, 1, 64), dict(new_lens=torch.zeros(2)), "new_lens"),
            (h(2, 2, 1, 64), h(2, 2, 1, 64), dict(new_lens=torch.zeros(3, dtype=torch.int32)), "new_lens"),
            (h(2, 2, 1, 64), h(2, 2, 1, 64), dict(new_lens=[1, 1]), "new_lens"),
            (h(2, 2, 1, 64, dt=torch.float16).to("meta"), h(2, 2, 1, 64).to("meta"), {}, "device")):
        with pytest.raises(ValueError, match=match):
            c.append(k_new, v_new, **kw)
    assert c.lens.tolist() == [0, 0]


def test_attention_value_errors_before_any_work():
    """The cache's own checks, and the keywords' ValueErrors of sageattn_qk_int8_pv_fp8_cuda, word for word the same functions."""
    c = _cache()
    q = torch.zeros(2, 4, 1, 64, dtype=torch.float16)
    for args, kw, match in (
            ((q.float(), c), {}, "dtype"),
            ((q.to("meta"), c), {}, "device"),
            ((torch.zeros(3, 4, 1, 64, dtype=torch.float16), c), {}, "B, D"),
            ((torch.zeros(2, 4, 1, 128, dtype=torch.float16), c), {}, "B, D"),
            ((torch.zeros(2, 3, 1, 64, dtype=torch.float16), c), {}, "divisible"),
            ((torch.zeros(2, 4, 64, dtype=torch.float16), c), {}, "4-D"),
            ((q, "cache"), {}, "QuantizedKVCache"),
            ((q, _cache(seeded=False)), {}, "no statistics"),
            ((q, c), dict(tensor_layout="HDN"), "layout"),
            ((q, c), dict(causal_align="middle"), "causal_align"),
            ((q, c), dict(causal_align="bottom_right"), "needs is_causal=True"),
            ((q, c), dict(q_start=1), "needs is_causal=True"),
            ((q, c), dict(is_causal=True, q_start=1, causal_align="bottom_right"), "not both"),
            ((q, c), dict(is_causal=True, q_start=torch.zeros(3, dtype=torch.int32)), r"shape \[B\]"),
            ((q, c), dict(window_size=(70,)), "window_size"),
            ((q, c), dict(window_size=(70, -1)), "window_size"),
            ((q, c), dict(is_causal=True, window_size=(70, 5)), "window_size"),
            ((q, c), dict(pack_gqa=1), "pack_gqa"),
            ((torch.zeros(2, 4, 33, 64, dtype=torch.float16), c), dict(pack_gqa=True), "qo_len <= 32"),
            ((torch.zeros(2, 2, 1, 64, dtype=torch.float16), c), dict(pack_gqa=True), "no GQA group"),
            ((q, c), dict(num_splits=256), "num_splits"),
            ((q, c), dict(num_splits=True), "num_splits"),
            ((torch.zeros(2, 4, 129, 64, dtype=torch.float16), c), dict(num_splits=2), "qo_len <= 128"),
            ((q, c), dict(num_splits=2, is_causal=True, window_size=(70, 0)), "num_splits cannot be combined")):
        with pytest.raises(ValueError, match=match):
            sageattn_kvcache(*args, **kw)


def test_from_prefill_value_errors():
    k = torch.zeros(2, 2, 8, 64, dtype=torch.float16)
    long = torch.zeros(2, 2, 72, 64, dtype=torch.float16)
    for args, kw in (((k, k[:, :, :4], 64), {}), ((k, k.bfloat16(), 64), {}), ((k[0], k[0], 64), {}), ((k, k, 64), dict(v_headroom=0.0)),
                     ((k, k, 64), dict(v_headroom=float("inf"))), ((k, k, 64), dict(kv_lens=torch.zeros(3, dtype=torch.int32))),
                     ((k, k, 64), dict(kv_lens=torch.zeros(2))), ((k, k, 0), {}), ((k, k, 64), dict(tensor_layout="HDN")),
                     ((long, long, 64), {})):        # 72 rows do not fit into 64
        with pytest.raises(ValueError):
            QuantizedKVCache.from_prefill(*args, **kw)


def test_the_random_append_schedules_reach_what_they_are_for():
    """The eight schedules tests/test_gpu_kv_cache.py checks after every step (B 4, capacity 320): every T, counts below 0 and above T, all
    three kinds of new_lens, a step that crosses a block end, one that ends on one, a sample without rows."""
    B, cap = 4, 320
    seen_t, kinds, flags = set(), set(), set()
    for seed in util.APPEND_SCHEDULE_SEEDS:
        final, steps = util.random_append_schedule(seed, B, cap)
        assert (final, steps) == util.random_append_schedule(seed, B, cap)
        have = [0] * B
        flags |= {"empty"} if 0 in final else set()
        for T, counts, kind in steps:
            seen_t.add(T)
            kinds.add(kind)
            assert kind != "none" or counts == (T,) * B
            for b, n in enumerate(counts):
                take = max(0, min(n, T))
                flags |= {"below"} if n < 0 else {"above"} if n > T else set()
                if take and (have[b] + take) % 64 == 0:
                    flags.add("ends_on_a_block_end")
                if take and have[b] // 64 != (have[b] + take - 1) // 64 and have[b] % 64:
                    flags.add("crosses_a_block_end")
                have[b] += take
        assert tuple(have) == final and all(0 <= n <= cap for n in final)
    assert seen_t == set(util.APPEND_SCHEDULE_TS) and kinds == {"i32", "i64", "none"}, (seen_t, kinds)
    assert flags >= {"below", "above", "ends_on_a_block_end", "crosses_a_block_end", "empty"}, flags
