"""CPU: the interface of the kv_lens family's exact split (``num_splits=``: a call of one query block as S key-range chunks) -- the keyword's
argument errors raised before any GPU work, the torch.compile refusal, the flag SAGE_ATTR_KV_SPLIT and the chunk count in flags bits 16-23
(their values, which entry point takes them and with which arguments, that the ABI is what it was), the workspace size against the header's
formula, the chunk arithmetic the three launches share, and the build of the kernels behind pass 2 (units sage_attn_d{128,64}_f8ks.hip:
instantiation count, names, zero scratch, the family's occupancy, the MFMA hazard lint)."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

import util  # noqa: F401  (sys.path)
import test_build_resources as tbr
import test_cabi_attn_rejects as rej
from sageattention_amd import _cabi, core as sc
from test_cabi import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("sage_attn_d128_f8ks.hip", "sage_attn_d64_f8ks.hip")
HONOURED = rej.KVLENS
FLAG = b"SAGE_ATTR_KV_SPLIT"


def _cpu_qkv(B=2, Hq=8, Hkv=2, Lq=16, Lk=256, D=64):
    z = lambda h, L: torch.zeros(B, h, L, D, dtype=torch.float16)
    return z(Hq, Lq), z(Hkv, Lk), z(Hkv, Lk)


def _lens(B=2):
    return torch.full((B,), 100, dtype=torch.int32)


ROUTES = [dict(), dict(kv_lens=_lens()), dict(is_causal=True), dict(is_causal=True, kv_lens=_lens()),
          dict(is_causal=True, causal_align="bottom_right", kv_lens=_lens()), dict(is_causal=True, q_start=_lens()),
          dict(pack_gqa=True), dict(pack_gqa=True, is_causal=True, causal_align="bottom_right", kv_lens=_lens())]
ROUTE_IDS = ["plain", "kv_lens", "causal", "causal_kv_lens", "bottom_right", "q_start", "pack_gqa", "pack_gqa_bottom_right"]


# ---------------------------------------------------------------------------------------------- Python: argument errors
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("kw,msg", [
    (dict(qk_quant_gran="per_warp"), "qk_quant_gran"),
    (dict(qk_quant_gran="per_block"), "qk_quant_gran"),
    (dict(pv_accum_dtype="fp32"), "pv_accum_dtype"),
    (dict(fuse_q_quant=False), "fuse_q_quant"),
    (dict(fp8_scores="folded"), "fp8_scores"),
    (dict(smooth_v=True), "smooth_v"),
    (dict(split_kv=2), "split_kv"),
    (dict(split_kv="auto"), "split_kv"),
    (dict(split_kv_exact=True), "split_kv_exact"),
])
@pytest.mark.parametrize("splits", [4, "auto"])
def test_refused_options_name_themselves_and_the_keyword(route, kw, msg, splits):
    """Everything the kv_lens route refuses is refused with ``num_splits`` too, whichever other keywords of the route the call carries, and the
    message names ``num_splits`` (its check runs first)."""
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match=msg) as e:
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, num_splits=splits, **route, **kw)
    assert "num_splits" in str(e.value)


@pytest.mark.parametrize("route", ROUTES[:6], ids=ROUTE_IDS[:6])
def test_more_than_one_query_block_raises(route):
    for Lq in (129, 256, 1000):
        q, k, v = _cpu_qkv(Lq=Lq)
        with pytest.raises(ValueError, match="num_splits needs qo_len <= 128"):
            sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, num_splits=2, **route)
    qn, kn, vn = (t.transpose(1, 2).contiguous() for t in _cpu_qkv(Lq=128))          # NHD: the row count is read per layout
    with pytest.raises(AssertionError, match="cuda"):
        sc.sageattn_qk_int8_pv_fp8_cuda(qn, kn, vn, tensor_layout="NHD", num_splits=2, **route)


@pytest.mark.parametrize("window,causal", [((100, 0), True), ((0, 0), True), ((5, -1), True), ((100, 7), False), ((0, 0), False)])
def test_a_window_that_bounds_the_look_back_raises(window, causal):
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match="num_splits cannot be combined with window_size"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, num_splits=2, is_causal=causal, window_size=window)
    for unbounded, c in (((-1, -1), False), ((-1, 0), True), ((-1, 5), False), (None, True)):       # no look-back bound: accepted
        with pytest.raises(AssertionError, match="cuda"):
            sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, num_splits=2, is_causal=c, window_size=unbounded)


@pytest.mark.parametrize("bad", [True, False, -1, 256, 1000, 2.0, "Auto", "yes", "4", [4], (2,)])
def test_the_keyword_is_an_int_in_range_or_auto(bad):
    q, k, v = _cpu_qkv()
    with pytest.raises(ValueError, match="num_splits must be None, an int in \\[0, 255\\] or 'auto'"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, num_splits=bad)


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("splits", [0, 2, 17, 255, "auto"])
def test_supported_calls_pass_the_argument_check(route, splits):
    for Lq in (1, 32) if route.get("pack_gqa") else (1, 33, 128):
        q, k, v = _cpu_qkv(Lq=Lq)
        for kw in (dict(), dict(pv_accum_dtype="fp32+fp32", smooth_k=False, split_kv=0)):
            with pytest.raises(AssertionError, match="cuda"):        # (accepted; then the ordinary input check of a CPU tensor)
                sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, num_splits=splits, **route, **kw)


def test_pack_gqa_keeps_its_own_rules_under_the_keyword():
    q, k, v = _cpu_qkv(Lq=33)
    with pytest.raises(ValueError, match="pack_gqa needs qo_len <= 32"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, num_splits=2, pack_gqa=True)
    q, k, v = _cpu_qkv(Hq=2, Hkv=2)
    with pytest.raises(ValueError, match="pack_gqa needs num_qo_heads / num_kv_heads >= 2"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, num_splits=2, pack_gqa=True)


@pytest.mark.parametrize("off", [None, 1])
def test_off_is_the_call_without_the_keyword(off):
    """None / 1 ask for nothing: no restriction of the route applies (more than one query block, the folded score form, a window ...) and
    the argument check returns 0, the value of a call without the keyword (bits and grid on the GPU: test_gpu_kv_split.py)."""
    q, k, v = _cpu_qkv(Hq=2, Hkv=2, Lq=300)
    with pytest.raises(AssertionError, match="cuda"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, num_splits=off, fp8_scores="folded", pv_accum_dtype="fp32")
    assert sc._num_splits_args(off, q, k, "HND", (5, 0), None, "per_warp", "fp32", True, dict(split_kv=3)) == 0
    assert inspect.signature(sc._attn_fused_q).parameters["num_splits"].default == 0


def test_torch_compile_refuses_the_keyword(monkeypatch):
    q, k, v = _cpu_qkv()
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    for fn in (sc.sageattn_qk_int8_pv_fp8_cuda, sc.sageattn):
        for splits in (2, "auto", 0):
            with pytest.raises(ValueError, match="num_splits is not supported under torch.compile"):
                fn(q, k, v, num_splits=splits)


def test_the_keyword_is_a_named_parameter_and_sageattn_forwards_it():
    for fn in (sc.sageattn_qk_int8_pv_fp8_cuda, sc.sageattn):
        par = inspect.signature(fn).parameters
        assert par["num_splits"].default is None and list(par)[-1] == "kwargs"
        assert "num_splits" in fn.__doc__
    assert "num_splits=num_splits" in inspect.getsource(sc.sageattn)
    q, k, v = _cpu_qkv(Lq=129)
    with pytest.raises(ValueError, match="num_splits needs qo_len <= 128"):       # checked before any work (not the input check's "cuda") ...
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, num_splits=2)
    with pytest.raises(ValueError, match="num_splits needs qo_len <= 128"):       # ... and first: pack_gqa's rule (qo_len <= 32) is broken too
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, num_splits=2, pack_gqa=True)


def test_the_auto_plan():
    """From B, Hq, Hkv, Lq, Lk alone.  No split above 64 unsplit workgroups, below 8192 or above 65536 keys, above 32 query rows; else the smallest S that reaches 512 workgroups,
    no chunk shorter than eight tiles, S in [8, 32] -- the region in which tools/num_splits_probe.py measured the route faster."""
    plan = sc._num_splits_plan
    assert plan(4, 32, 8, 1, 8192, True) == 16                   # DESIGN 3.14's shape: 32 packed workgroups, 128 tiles
    assert plan(1, 32, 8, 16, 65536, True) == 32                 # 8 packed workgroups: 64 chunks would reach 512, 32 is the largest measured
    assert plan(1, 32, 8, 1, 65536, False) == 16                 # unpacked: 32 workgroups
    assert plan(8, 32, 8, 1, 65536, True) == 8 and plan(2, 32, 8, 1, 8192, False) == 8           # 64 workgroups
    assert plan(16, 32, 8, 1, 65536, True) == 0 and plan(4, 32, 8, 128, 65536, False) == 0       # 128 workgroups: no chunk count was faster
    assert plan(32, 32, 8, 1, 65536, True) == 0 and plan(9, 8, 8, 1, 65536, False) == 0
    assert plan(1, 8, 8, 1, 8192, False) == 16 and plan(1, 8, 8, 1, 8191, False) == 0            # below the shortest key range measured
    assert plan(1, 1, 1, 1, 65536, False) == 32 and plan(1, 1, 1, 1, 65537, False) == 0 and plan(1, 1, 1, 1, 10 ** 6, False) == 0      # above the longest measured
    assert plan(1, 32, 8, 32, 65536, True) == 32 and plan(1, 32, 8, 33, 65536, False) == 0 and plan(1, 32, 8, 128, 65536, False) == 0  # decode shapes only
    for B in range(1, 40):
        for Hq, Hkv in ((32, 8), (8, 8), (5, 1), (64, 8)):
            for Lk in (1, 1061, 8192, 10000, 32768, 65536, 10 ** 6):
                for packed in (False, True):
                    Lq = (1, 16, 32, 33)[(B + Lk) % 4]
                    S = plan(B, Hq, Hkv, Lq, Lk, packed)
                    wgs = B * Hkv * ((Hq // Hkv + 3) // 4) if packed else B * Hq
                    assert S == 0 or (8 <= S <= 32 and wgs <= 64 and 8192 <= Lk <= 65536 and Lq <= 32 and ((Lk + 63) // 64) // S >= 8 and wgs * (S - 1) < 512), (B, Hq, Hkv, Lk, S)


# ---------------------------------------------------------------------------------------------- C ABI: the flag and the count
def test_the_defines_equal_their_mirrors_and_the_abi_is_unchanged():
    lib = _cabi.load()
    header = open(os.path.join(ROOT, "include", "sage_gfx950.h")).read()
    m = re.search(r"^#define\s+SAGE_ATTR_KV_SPLIT\s+0x([0-9a-fA-F]+)u\s*$", header, re.M)
    assert m and int(m.group(1), 16) == _cabi.ATTR_KV_SPLIT == 0x800
    m = re.search(r"^#define\s+SAGE_ATTR_KV_SPLIT_SHIFT\s+(\d+)\s*$", header, re.M)
    assert m and int(m.group(1)) == _cabi.ATTR_KV_SPLIT_SHIFT == 16
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22 and len(prototypes()) == 56 and len(_cabi.SYMBOLS) == 56
    assert ctypes.sizeof(_cabi.SageLaunchAttr) == 56 and [f[0] for f in _cabi.SageLaunchAttr._fields_][-2:] == ["window", "q_start"]
    assert _cabi.SageLaunchAttr.window.offset == 44 and _cabi.SageLaunchAttr.q_start.offset == 48 and len(rej.ATTN) == 17
    assert re.search(r"^ \*  flags bit 0x800\s+SAGE_ATTR_KV_SPLIT", header, re.M), "the header's attribute block documents the flag"
    block = header[header.index(" *  flags bit 0x800"):header.index("typedef struct SageLaunchAttr")]
    for piece in ("flags bits 16-23", "SPLIT WORKSPACE", "chunk_max [B, Hkv, S, Hq / Hkv, Lq]", "lse_part [B, Hkv, S, Hq / Hkv, Lq]",
                  "o_part [B, Hkv, S, Hq / Hkv, Lq, D]", "grid_out reports pass 2's grid", "sage_attn_fused_q_pv_f8_kvlens alone"):
        assert piece in block, piece


def test_launch_attr_carries_the_flag_and_the_count():
    assert _cabi.launch_attr() is None and _cabi.launch_attr(kv_split=0) is None
    a = _cabi.launch_attr(kv_split=4)
    assert a is not None and a.flags == 0x800 | (4 << 16) and a.struct_bytes == 56 and a.window == 0 and not a.q_start and not a.launch_ws
    assert _cabi.launch_attr(kv_split=255, gqa_pack=True).flags == 0x900 | (255 << 16)
    for bad in (1, 256, -3, True):
        with pytest.raises(ValueError, match="kv_split"):
            _cabi.launch_attr(kv_split=bad)
    from sageattention_amd import ops
    par = inspect.signature(ops.attn_attr).parameters
    assert "kv_split" in par and "split_ws" in par


def _call(name, flags, launch_ws=None, launch_ws_bytes=0, window=0, **wrong):
    """``name`` with the refusal table's valid arguments (host memory: the library must refuse before its first HIP call) but for ``wrong``."""
    attr = _cabi.SageLaunchAttr(struct_bytes=ctypes.sizeof(_cabi.SageLaunchAttr), flags=flags, launch_ws=launch_ws, launch_ws_bytes=launch_ws_bytes,
                                window=window)
    args = []
    for ctype, pname in prototypes()[name][1]:
        args.append(wrong[pname] if pname in wrong else rej.VALID[pname] if pname in rej.VALID else rej.P)
    args[-1] = ctypes.byref(attr)
    lib = _cabi.load()
    return getattr(lib, name)(*args), lib.sage_last_error()


def _flags(S, *more):
    f = _cabi.ATTR_KV_SPLIT | (S << _cabi.ATTR_KV_SPLIT_SHIFT)
    for m in more:
        f |= m
    return f


@pytest.mark.parametrize("name", [n for n in rej.ATTN if n != HONOURED])
@pytest.mark.parametrize("causal", [0, 1])
def test_every_other_entry_point_refuses_the_flag_and_the_count_bits(name, causal):
    """Sixteen entries, the exact split's own attribute path included: the bit with a count, the bit alone, a count alone, each count bit alone."""
    kw = {} if name.endswith("_masked") else dict(is_causal=causal)
    for flags in (_flags(4), _cabi.ATTR_KV_SPLIT, 4 << 16, *(1 << b for b in range(16, 24))):
        for ws in (dict(), dict(launch_ws=rej.P, launch_ws_bytes=1 << 30)):
            rc, err = _call(name, flags, **ws, **kw)
            assert rc == -1 and FLAG in err, (hex(flags), rc, err)


def test_sixteen_entries_refuse_and_one_honours():
    assert HONOURED in rej.ATTN and len([n for n in rej.ATTN if n != HONOURED]) == 16 and rej.EXACT in rej.ATTN


BIG = dict(launch_ws=rej.P, launch_ws_bytes=1 << 40)


@pytest.mark.parametrize("causal", [0, 1])
def test_the_honoured_entry_refuses_what_the_route_does_not_take(causal):
    cases = [
        (_flags(0), BIG, dict(), b"2 .. 255"), (_flags(1), BIG, dict(), b"2 .. 255"),            # S outside [2, 255]
        (4 << 16, BIG, dict(), b"without the bit"), (1 << 23, dict(), dict(), b"without the bit"),   # a count without the flag
        (_flags(4), BIG, dict(Lq=129), b"Lq <= 128"), (_flags(4), BIG, dict(Lq=4096), b"Lq <= 128"),
        (_flags(4, _cabi.ATTR_FP8_FOLDED_SCORES), BIG, dict(), b"exact score form"),
        (_flags(4, _cabi.ATTR_FORCE_PERSISTENT), BIG, dict(), FLAG),
        (_flags(4), BIG, dict(v_mean=rej.P), b"v_mean"),                                             # a V mean is added per chunk: refused
        (_flags(4), dict(), dict(), b"split workspace"),                                             # null
        (_flags(4), dict(launch_ws=rej.P + 64, launch_ws_bytes=1 << 40), dict(), b"128-byte aligned"),
        (_flags(4), dict(launch_ws=rej.P, launch_ws_bytes=_cabi.kv_split_ws_bytes(1, 4, 128, 64, 4) - 1), dict(), b"split workspace"),
        (_flags(4), dict(launch_ws=rej.P, launch_ws_bytes=4096), dict(), b"split workspace"),      # a ticket block is not one
    ]
    for flags, ws, wrong, piece in cases:
        rc, err = _call(HONOURED, flags, is_causal=causal, **ws, **wrong)
        assert rc == -1 and FLAG in err and piece in err, (hex(flags), wrong, rc, err)
    rc, err = _call(HONOURED, _flags(4), is_causal=1, window=100, **BIG)
    assert rc == -1 and FLAG in err and b"no window" in err, (rc, err)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("S", [2, 17, 255])
def test_the_honoured_entry_takes_the_flag_as_far_as_the_checks_go(causal, S):
    """The next refusal is the one asked for (head_dim 96), not the flag's -- the tensors are host memory; with SAGE_ATTR_GQA_PACK and decode
    rows as well."""
    for flags, shape in ((_flags(S), dict()), (_flags(S), dict(Lq=1)), (_flags(S, _cabi.ATTR_GQA_PACK), dict(Lq=16)),
                         (_flags(S, _cabi.ATTR_FP8_EXACT_SCORES), dict(Lq=33))):
        rc, err = _call(HONOURED, flags, is_causal=causal, D=96, **BIG, **shape)
        assert rc == -1 and b"head_dim must be 64 or 128 (got 96)" in err and FLAG not in err, (rc, err)


@pytest.mark.parametrize("name", rej.ATTN)
def test_the_bits_around_stay_unknown(name):
    for bit in (0x10, 0x20, 0x40, 0x80, 0x200, 0x400, 0x1000, 0x8000, 1 << 24, 1 << 31):
        for flags in (bit, bit | _flags(4)):
            rc, err = _call(name, flags, **BIG, **({} if name.endswith("_masked") else dict(is_causal=1)))
            assert rc == -1 and b"unknown SageLaunchAttr.flags" in err, (name, hex(flags), rc, err)


# ---------------------------------------------------------------------------------------------- the workspace
def test_workspace_bytes_follow_the_headers_formula():
    header = open(os.path.join(ROOT, "include", "sage_gfx950.h")).read()
    m = re.search(r"bytes = (2 \* r128\(4 \* B \* Hq \* S \* Lq\) \+ r128\(4 \* B \* Hq \* S \* Lq \* D\)),\s+r128\(x\) = \(x \+ 127\) / 128 \* 128", header)
    assert m, "the header states the byte formula"
    r128 = lambda x: (x + 127) // 128 * 128
    for B, Hq, Lq, D, S in ((1, 4, 128, 64, 4), (6, 5, 1, 128, 17), (3, 6, 5, 64, 2), (1, 1, 1, 64, 255), (2, 32, 33, 128, 16), (4, 32, 16, 128, 32)):
        want = eval(m.group(1), dict(r128=r128, B=B, Hq=Hq, Lq=Lq, D=D, S=S))
        got = _cabi.kv_split_ws_bytes(B, Hq, Lq, D, S)
        assert got == want and got % 128 == 0, (B, Hq, Lq, D, S, got, want)
        rows = B * Hq * S * Lq
        assert got >= 4 * rows * (D + 2) and got - 4 * rows * (D + 2) < 3 * 128
    # ... and the library asks for the same number: one byte less is refused, naming it
    need = _cabi.kv_split_ws_bytes(1, 4, 128, 64, 4)
    rc, err = _call(HONOURED, _flags(4), launch_ws=rej.P, launch_ws_bytes=need - 1)
    assert rc == -1 and f"{need} bytes".encode() in err, (need, err)
    rc, err = _call(HONOURED, _flags(17, _cabi.ATTR_GQA_PACK), launch_ws=rej.P, launch_ws_bytes=0, Lq=5)
    assert rc == -1 and f"{_cabi.kv_split_ws_bytes(1, 4, 5, 64, 17)} bytes".encode() in err, err


# ---------------------------------------------------------------------------------------------- the chunk arithmetic
def _cdiv(a, b):
    """C's integer division (truncation towards zero), as the kernel's signed bounds are formed."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def _chunks(Lk, S, length, start, Lq, causal):
    """What pass 2's work items (sage_attn_kernel.h, SEED with KVLEN) form for each chunk of one sample: (first key, keys, tiles requested),
    then per row the global keys it sees in the chunk."""
    T = ((Lk + 63) // 64 + S - 1) // S
    n = max(0, min(length, Lk))
    s = max(-Lq, min(start, Lk))
    out = []
    for c in range(S):
        kc0 = 64 * T * c
        lk = max(0, min(n - kc0, 64 * T))
        kchunk0 = kc0 - s
        tiles = (lk + 63) // 64
        if causal:
            tiles = min(tiles, max(0, _cdiv(128 - kchunk0 + 63, 64)))
        seen = []
        for i in range(Lq):
            hi = min(lk, 64 * tiles)
            if causal:
                hi = min(hi, i - kchunk0 + 1)
            seen.append(range(kc0, kc0 + max(0, hi)))
        out.append((kc0, lk, tiles, seen))
    return T, n, s, out


SWEEP = [(Lk, S, length, start, Lq) for Lk in (1, 65, 1061, 4096) for S in (2, 4, 16, 17, 255) for length in (0, 1, 64, 320, 321, 700, 1061, 5000, -4)
         for start in (0, -3, 300, 1000, -200, 10 ** 6) for Lq in (1, 5, 33, 128)]


def _rows(Lq):
    return range(Lq) if Lq <= 33 else (0, 1, 31, 32, 63, 64, 126, 127)


def test_the_chunks_partition_the_visible_keys():
    """For every (Lk, S, len, offset, Lq), non-causal and causal: the chunks hold every visible key of every row exactly once; a chunk that
    requests a tile starts inside the tensor and inside the sample and requests no tile from ceil(len / 64) on; the chunks that request no
    tile are exactly those in which the query block (its 128 row slots, as the unsplit kernel bounds its loop) sees no key."""
    for Lk, S, length, start, Lq in SWEEP:
        for causal in (False, True):
            T, n, s, chunks = _chunks(Lk, S, length, start, Lq, causal)
            assert T >= 1 and S * T >= (Lk + 63) // 64
            for i in _rows(Lq):
                want_end = max(0, min(n, s + i + 1) if causal else n)
                pos = 0                                          # the chunks' key ranges, in order, tile [0, want_end) without gap or overlap
                for c in chunks:
                    r = c[3][i]
                    if len(r):
                        assert r.start == pos, (Lk, S, length, start, Lq, causal, i)
                        pos = r.stop
                assert pos == want_end, (Lk, S, length, start, Lq, causal, i)
            for kc0, lk, tiles, _ in chunks:
                block_sees = lk > 0 and (not causal or 127 - (kc0 - s) >= 0)
                assert (tiles > 0) == block_sees, (Lk, S, length, start, Lq, causal, kc0)
                if tiles:
                    assert kc0 < n <= Lk and kc0 + 64 * tiles <= 64 * ((n + 63) // 64), (Lk, S, length, start, causal, kc0, tiles)


def test_pass1_and_pass2_agree_on_the_tiles_of_a_chunk():
    """Pass 1 (sage_split_exact.hip, chunk_max_lens_kernel) bounds a wave's tiles by its last row that exists; they are a prefix of pass 2's
    and hold every key a row of the wave sees."""
    for Lk, S, length, start, Lq in SWEEP[::7]:
        T, n, s, chunks = _chunks(Lk, S, length, start, Lq, True)
        nt = (n + 63) // 64
        for c, (kc0, lk, tiles, seen) in enumerate(chunks):
            for row0 in range(0, Lq, 32):
                rlast = min(row0 + 31, Lq - 1)
                vis = s + rlast
                t0, t1 = c * T, min(c * T + T, nt, vis // 64 + 1 if vis >= 0 else 0)
                assert t1 - t0 <= tiles
                for i in range(row0, rlast + 1):
                    r = seen[i]
                    assert not len(r) or (64 * t0 <= r.start and r.stop <= 64 * t1), (Lk, S, length, start, Lq, c, i)


# ---------------------------------------------------------------------------------------------- the build
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_kv_split_units_build_within_the_family_targets():
    """The units are in the Makefile's SRCS and cross-compile for gfx950; each holds eight kernels -- fp16 / bf16 q x {non-causal lengths, causal
    offsets} x {unpacked, packed} -- whose forms are the KVLEN kernels' with the SEED flag set: zero scratch, no spilled VGPR or SGPR,
    D = 128 at two waves per SIMD, D = 64 at three."""
    mk = open(os.path.join(ROOT, "sageattention_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert all(u in srcs for u in UNITS), srcs
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as ex:
        reports = dict(zip(UNITS, ex.map(tbr._resource_report, UNITS)))
    for unit, rep in reports.items():
        mine = {k: v for k, v in rep.items() if "sage_attn_kernel" in k}
        assert len(mine) == 8, (unit, sorted(mine))
        d128 = "d128" in unit
        forms = set()
        for name, res in mine.items():
            # D, FP8 PV, causal or not, per-thread k scales, two-level, no mask, QF 1 / 2, GPACK or not, the exact form, no CPERS / VROWS, SEED, no WINDOW, QSTART = causal, KVLEN
            f = tbr.kf.decode(name)
            assert f["qf"] in (1, 2) and f == tbr.kf.form(128 if d128 else 64, pv_fp8=True, kthread=True, two_level=True, seed=True, kvlen=True,
                                                          causal=f["causal"], qstart=f["causal"], qf=f["qf"], gpack=f["gpack"]), name
            forms.add((f["causal"], f["qf"], f["gpack"]))
            assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0 and res["ScratchSize"] == 0, (name, res)
            assert res["Occupancy"] >= (2 if d128 else 3) and res["VGPRs"] <= (256 if d128 else 168), (name, res)
        assert forms == {(c, f, g) for c in (False, True) for f in (1, 2) for g in (False, True)}, sorted(forms)       # (causal, QF, GPACK)


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_pass1_kernels_build_without_scratch():
    rep = tbr._resource_report("sage_split_exact.hip")
    mine = {k: v for k, v in rep.items() if "chunk_max_lens_kernel" in k}
    assert len(mine) == 8 and len([k for k in rep if "chunk_max_kernel" in k]) == 8, sorted(rep)
    for name, res in mine.items():
        assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0 and res["Occupancy"] >= 2, (name, res)


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_kv_split_units_pass_the_mfma_hazard_lint():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_hazard_lint as lint
    assert lint.UNITS_KV_SPLIT == UNITS
    assert not set(UNITS) & set(lint.UNITS + lint.UNITS_PAIR + lint.UNITS_WINDOW + lint.UNITS_PACKED_BR + lint.UNITS_PACKED_WINDOW + lint.UNITS_GQA_PACK)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as ex:
        results = dict(zip(UNITS, ex.map(lambda u: lint.lint(lint.listing(u)), UNITS)))
    for unit, (findings, n_mfma) in results.items():
        assert n_mfma >= 400, (unit, n_mfma)                   # (eight kernels: the walk did see the pipelined loops)
        assert not findings, (unit, findings[:5])
