"""CPU: the step call on the paged KV cache -- C boundary, Python interface, the band filter, the build (include/sage_kvstep_gfx950.h,
sageattention_amd/_cabi_kvstep.py, sageattention_amd/paged_kv_step.py, csrc/sage_ragged.h, csrc/sage_attn_d{128,64}_{f8pb,f8pbg}.hip).  The new
header's prototypes are the new binding's table, the library exports them, every argument error of the entry returns -1 with its message before
anything touches a GPU and in the header's order, the Python layer raises ValueError before any work, the two bands partition what the clamp
yields over hostile words (a stand-alone program under AddressSanitizer and UBSan), each new unit holds exactly the step kernels of the forms it
is instantiated from, without scratch and at its form's occupancy -- and none of it moved what the other headers, bindings and units pin."""
import ctypes
import itertools
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import util  # noqa: F401  (sys.path)
import sageattention_amd as sa
import test_build_resources as tbr
import test_kv_varlen_host as varlen
import test_paged_kv_host as paged
from sageattention_amd import _cabi, _cabi_kvcache, _cabi_kvfork, _cabi_kvpaged, _cabi_kvpsplit, _cabi_kvpvarlen, _cabi_kvstep
from sageattention_amd.kv_cache import QuantizedKVCache
from sageattention_amd.paged_kv_step import sageattn_kvcache_step
from sageattention_amd.paged_kv_varlen import sageattn_kvcache_varlen
from test_kv_cache_host import MAIN_HEADER, _prototypes, _text
from test_paged_kv_host import listed  # noqa: F401  (the fixture: the forms of the lists the paged, the ragged and the step units are instantiated from)

kf = tbr.kf
ROOT = tbr.ROOT
CSRC = os.path.join(ROOT, "sageattention_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "sage_kvstep_gfx950.h")
ENTRIES = ["sage_kvstep_abi_version", "sage_kvstep_attn"]
_Dev = varlen._Dev


def test_binding_is_the_header():
    protos = _prototypes(HEADER, "SAGE_KVSTEP_API")
    assert sorted(protos) == sorted(_cabi_kvstep.SYMBOLS) == ENTRIES
    for name, (ret, params) in protos.items():
        res, argtypes = _cabi_kvstep.SYMBOLS[name]
        assert res is paged._ctype(ret), f"{name}: returns {ret}, bound as {res}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters declared, {len(argtypes)} bound"
        for i, (ctype, bound) in enumerate(zip(params, argtypes)):
            assert bound is paged._ctype(ctype), f"{name}: parameter {i} ({ctype}) bound as {bound}"
    version = int(re.search(r"#define\s+SAGE_KVSTEP_ABI_VERSION\s+(\d+)", _text(HEADER)).group(1))
    assert version == 1 == _cabi_kvstep.ABI_VERSION
    rest = re.sub(r"SAGE_KVSTEP_API", "", _text(HEADER))
    assert "SAGE_API" not in rest and "SAGE_KVPAGED_API" not in rest and "SAGE_KVPVARLEN_API" not in rest          # an export macro of its own
    assert "sage_kvstep_gfx950.h" in open(os.path.join(CSRC, "Makefile")).read()
    # the entry takes sage_kvpvarlen_attn's arguments, argument for argument
    theirs = _prototypes(varlen.HEADER, "SAGE_KVPVARLEN_API")["sage_kvpvarlen_attn"]
    assert protos["sage_kvstep_attn"] == theirs and _cabi_kvstep.SYMBOLS["sage_kvstep_attn"] == _cabi_kvpvarlen.SYMBOLS["sage_kvpvarlen_attn"]


def test_library_exports_the_entries_and_the_other_boundaries_did_not_move():
    lib = ctypes.CDLL(_cabi.LIB_PATH)
    for name in _cabi_kvstep.SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
    assert _cabi_kvstep.load() is _cabi.load()                       # one library, bound behind _cabi.load()
    assert _cabi_kvstep.load().sage_kvstep_abi_version() == 1
    assert _cabi.ABI_VERSION == 22 and lib.sage_abi_version() == 22
    assert len(_prototypes(MAIN_HEADER, "SAGE_API")) == 56 and len(_cabi.SYMBOLS) == 56
    assert sorted(_cabi_kvpvarlen.SYMBOLS) == varlen.ENTRIES and len(varlen.ENTRIES) == 3 and _cabi_kvpvarlen.load().sage_kvpvarlen_abi_version() == 1
    assert sorted(_prototypes(varlen.HEADER, "SAGE_KVPVARLEN_API")) == varlen.ENTRIES
    assert sorted(_cabi_kvpaged.SYMBOLS) == paged.ENTRIES and _cabi_kvpaged.load().sage_kvpaged_abi_version() == 1
    assert _cabi_kvcache.load().sage_kvcache_abi_version() == 1 and _cabi_kvfork.load().sage_kvfork_abi_version() == _cabi_kvfork.ABI_VERSION
    assert _cabi_kvpsplit.load().sage_kvpsplit_abi_version() == _cabi_kvpsplit.ABI_VERSION
    others = [n for b in (_cabi, _cabi_kvcache, _cabi_kvpaged, _cabi_kvfork, _cabi_kvpsplit, _cabi_kvpvarlen) for n in b.SYMBOLS]
    assert not any(n.startswith("sage_kvstep") for n in others)
    assert not hasattr(sa, "sageattn_kvcache_step") and "sageattn_kvcache_step" not in sa.__all__


# ---- argument errors of the entry, in the header's order ------------------------------------------------------------------------------------
_DEFAULT = object()


def _attn(lib, p, attr=_DEFAULT, **kw):
    a = dict(q=p, k_int8=p, v_image=p, o=p, lse=None, k_scale=p, v_scale=p, kv_lens=p, cu_seqlens_q=p, block_table=p, bt_stride=2, num_pages=4,
             page_size=64, max_pages_per_seq=2, B=1, Hq=2, Hkv=1, total_q=1, max_seqlen_q=1, D=64, q_sl=128, q_sh=64, k_sb=4096, k_sh=4096, k_sl=64,
             o_sl=128, o_sh=64, lse_sh=1, is_causal=1, sm_scale_log2=1.0, q_dtype=0, out_dtype=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    if attr is _DEFAULT:
        attr = _cabi.launch_attr(q_start=_Dev(p))
    return lib.sage_kvstep_attn(*a.values(), _cabi.attr_arg(attr)), lib.sage_last_error()


def _attn_order(p):
    e = b"sage_kvstep_attn: "
    return [(dict(q=None), e + b"null tensor pointer"),
            (dict(kv_lens=None), e + b"null kv_lens"),
            (dict(cu_seqlens_q=None), e + b"null cu_seqlens_q"),
            (dict(block_table=None), b"null block_table"),
            (dict(page_size=96), b"page_size must be 64 * 2^k"),
            (dict(num_pages=0), b"num_pages must be at least 1"),
            (dict(max_pages_per_seq=0), b"max_pages_per_seq must be at least 1"),
            (dict(B=0), b"B and Hkv"),
            (dict(block_table=p + 2), b"block_table must be 4-byte aligned"),
            (dict(cu_seqlens_q=p + 2), e + b"cu_seqlens_q must be 4-byte aligned"),
            (dict(total_q=0), e + b"total_q and max_seqlen_q must be at least 1"),
            (dict(is_causal=0), e + b"is_causal must be 1"),
            (dict(Hq=2 ** 20, max_seqlen_q=2 ** 20), e + b"B * Hq * ceil(max_seqlen_q / 128) must be in [1, 2^31)"),
            (dict(lse=p, lse_sh=0), e + b"lse is [Hq, total_q]: its head stride lse_sh must be at least total_q"),
            (dict(Hkv=2), e + b"Hq / Hkv must be at least 2, no GQA group to pack"),
            (dict(attr=_cabi.launch_attr(_Dev(p), kv_split=2, q_start=_Dev(p))), e + b"SAGE_ATTR_KV_SPLIT is not supported on a paged cache"),
            (dict(D=96), b"head_dim must be 64 or 128"),
            (dict(Hq=5, Hkv=2), b"divisible"),
            (dict(q_dtype=2), b"bad q_dtype"),
            (dict(out_dtype=-1), b"bad out_dtype"),
            (dict(o=p + 2), b"16-byte aligned"),
            (dict(q_sl=68), b"q strides"),
            (dict(k_sl=72), b"k strides"),
            (dict(o_sh=4), b"output strides")]


def test_every_argument_error_returns_minus_one_in_the_headers_order():
    lib = _cabi_kvstep.load()
    buf, p = paged._aligned_buffer()
    checks = _attn_order(p)
    for kw, match in checks:                                         # each violation alone gives its own message, under the entry's own name
        rc, msg = _attn(lib, p, **kw)
        assert rc == -1 and match in msg and b"sage_kvpvarlen" not in msg.replace(b"sage_kvpvarlen_attn takes such a call", b""), (kw, rc, msg)
    covered = set()
    for (i, (kw_i, match_i)), (j, (kw_j, _)) in itertools.combinations(enumerate(checks), 2):
        if set(kw_i) & set(kw_j):                                    # two values for one argument do not fit into one call
            continue
        rc, msg = _attn(lib, p, **kw_i, **kw_j)
        assert rc == -1 and match_i in msg, (kw_i, kw_j, rc, msg)
        covered.add((i, j))
    assert all((i, i + 1) in covered for i in range(len(checks) - 1)), sorted(covered)
    with pytest.raises(ValueError):
        _cabi.check(-1, "sage_kvstep_attn")
    # no group to pack: one query head per kv head, however many there are
    rc, msg = _attn(lib, p, Hq=4, Hkv=4)
    assert rc == -1 and b"sage_kvstep_attn: Hq / Hkv must be at least 2, no GQA group to pack (got Hq 4, Hkv 4" in msg
    rc, msg = _attn(lib, p, Hq=3, Hkv=2)
    assert rc == -1 and b"no GQA group to pack" in msg
    del buf


def test_the_attributes_the_entry_refuses_by_name():
    lib = _cabi_kvstep.load()
    buf, p = paged._aligned_buffer()
    ws, qs = _Dev(p), _Dev(p)
    e = b"sage_kvstep_attn: "
    for attr, match in ((_cabi.launch_attr(ws, kv_split=2, q_start=qs), e + b"SAGE_ATTR_KV_SPLIT is not supported on a paged cache"),
                        (_cabi.launch_attr(folded_scores=True, q_start=qs), e + b"SAGE_ATTR_FP8_FOLDED_SCORES is not supported on a paged cache"),
                        (_cabi.launch_attr(ws, force_persistent=True, q_start=qs), e + b"SAGE_ATTR_FORCE_PERSISTENT is not supported on a paged cache"),
                        (_cabi.launch_attr(gqa_pack=True, q_start=qs), e + b"SAGE_ATTR_GQA_PACK is not taken (the entry packs the decode rows of a GQA group on its own)"),
                        # ... in that order, and all of them in front of the missing offsets
                        (_cabi.launch_attr(folded_scores=True, gqa_pack=True), e + b"SAGE_ATTR_FP8_FOLDED_SCORES"),
                        (_cabi.launch_attr(gqa_pack=True), e + b"SAGE_ATTR_GQA_PACK"),
                        (_cabi.launch_attr(window=5), e + b"SageLaunchAttr.q_start is required"),
                        (None, e + b"SageLaunchAttr.q_start is required")):
        rc, msg = _attn(lib, p, attr=attr)
        assert rc == -1 and match in msg, (rc, msg)
    # max_seqlen_q above one wave's slab does not trip the dense rule of SAGE_ATTR_GQA_PACK (Lq <= 32): the next check answers, whatever
    # max_seqlen_q is
    for max_q in (1, 32, 33, 4096):
        rc, msg = _attn(lib, p, max_seqlen_q=max_q, D=96)
        assert rc == -1 and b"head_dim must be 64 or 128" in msg and b"GQA_PACK" not in msg, (max_q, msg)
    # the ragged entry's own messages kept their wording, and it still refuses the flag
    rc, msg = varlen._attn(_cabi_kvpvarlen.load(), p, attr=_cabi.launch_attr(gqa_pack=True, q_start=qs))
    assert rc == -1 and b"sage_kvpvarlen_attn: SAGE_ATTR_GQA_PACK is not supported on packed query rows (one workgroup per query head)" in msg
    rc, msg = varlen._attn(_cabi_kvpvarlen.load(), p, attr=None)
    assert rc == -1 and b"sage_kvpvarlen_attn: SageLaunchAttr.q_start is required (int32 [B]: the key position of each sample's row 0)" in msg
    rc, msg = varlen._attn(_cabi_kvpvarlen.load(), p, Hkv=2, D=96)             # ... and takes a call without a group
    assert rc == -1 and b"head_dim must be 64 or 128" in msg
    del buf


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------------
def test_value_errors_before_any_work():
    c = paged._cache(seeded=True)                # B 2, Hkv 2, D 64, fp16, pages of 128, on the CPU
    q = torch.zeros(5, 4, 64, dtype=torch.float16)
    cu = torch.tensor([0, 2, 5], dtype=torch.int32)
    contiguous = QuantizedKVCache.allocate(2, 2, 64, 64, torch.float16, "cpu")
    for args, kw, match in (
            ((q, contiguous, cu, 3), {}, "sageattn_kvcache_step takes a PagedQuantizedKVCache"),
            ((q, "cache", cu, 3), {}, "sageattn_kvcache_step takes a PagedQuantizedKVCache"),
            ((q, paged._cache(seeded=False), cu, 3), {}, "no statistics"),
            ((q[:, :2], c, cu, 3), {}, r"Hq / Hkv must be at least 2 \(got 2 / 2\)"),
            ((torch.zeros(5, 3, 64, dtype=torch.float16), c, cu, 3), {}, "divisible"),
            ((q.unsqueeze(0), c, cu, 3), {}, "3-D"),
            ((q.float(), c, cu, 3), {}, "dtype"),
            ((q.to("meta"), c, cu, 3), {}, "device"),
            ((torch.zeros(5, 4, 128, dtype=torch.float16), c, cu, 3), {}, "must be"),
            ((torch.zeros(0, 4, 64, dtype=torch.float16), c, cu, 3), {}, "must be"),
            ((q, c, cu.long(), 3), {}, "cu_seqlens_q must be an int32 tensor"),
            ((q, c, cu[:2], 3), {}, r"shape \[B \+ 1\]"),
            ((q, c, cu.to("meta"), 3), {}, "device"),
            ((q, c, cu, 0), {}, "max_seqlen_q must be a positive int"),
            ((q, c, cu, True), {}, "max_seqlen_q must be a positive int"),
            # the keywords that exist on the dense call: the family's one resolver, its messages
            ((q, c, cu, 3), dict(window_size=(70,)), "window_size"),
            ((q, c, cu, 3), dict(window_size=(70, 5)), "window_size"),
            ((q, c, cu, 3), dict(q_start=torch.zeros(3, dtype=torch.int32)), r"shape \[B\]"),
            ((q, c, cu, 3), dict(q_start=torch.zeros(2)), "q_start must be an int")):
        with pytest.raises(ValueError, match=match):
            sageattn_kvcache_step(*args, **kw)
    # keywords the call does not have stay away, and the ragged call still refuses pack_gqa
    for kw in (dict(pack_gqa=True), dict(num_splits=2)):
        with pytest.raises(TypeError):
            sageattn_kvcache_step(q, c, cu, 3, **kw)
    with pytest.raises(ValueError, match="pack_gqa is not supported by sageattn_kvcache_varlen"):
        sageattn_kvcache_varlen(q, c, cu, 3, pack_gqa=True)


# ---- the band filter ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_bands_partition_the_clamp_over_hostile_prefix_words_under_the_sanitizers(tmp_path):
    """tests/ragged_band_main.cpp: a program of its own (no GPU, nothing loaded into this process), AddressSanitizer and UBSan on the host."""
    exe = tmp_path / "ragged_band"
    # (host code only: every sanitizer option goes to the host compilation by name, none reaches a device code object)
    host = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    out = subprocess.run([tbr.HIPCC, "-std=c++17", "-O1", "-g", *host, "-I", CSRC,
                          os.path.join(ROOT, "tests", "ragged_band_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    syms = subprocess.run(["nm", str(exe)], capture_output=True, text=True, timeout=60).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the program was built without the sanitizers"
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "all inside, none twice" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, \
        (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    # the kernels and the program read one definition; the body's two ragged_rows sites are what they were, the band site is a third name
    ragged = open(os.path.join(CSRC, "sage_ragged.h")).read()
    assert "inline void ragged_band(int c0, int c1, int total, int max_rows, int lo, int hi, int &first, int &rows)" in ragged
    body = open(os.path.join(CSRC, "sage_attn_body.h")).read()
    assert body.count("ragged_rows(") == 2 and body.count("ragged_band(") == 1
    kernel_h = open(os.path.join(CSRC, "sage_attn_kernel.h")).read()
    assert kernel_h.count("#define SAGE_ATTN_BODY_BAND false") == 3 and kernel_h.count("#define SAGE_ATTN_BODY_BAND true") == 1


# ---- the build ------------------------------------------------------------------------------------------------------------------------------
STEP_UNITS = {"f8pb": ("UNIT_F8Q", "UNIT_F8W"), "f8pbg": ("UNIT_F8G",)}
STEP_NAME = r"_ZN4sage27sage_attn_paged_step_kernelILj(\d+)EEEvNS_10AttnParamsENS_9PagedArgsENS_10RaggedArgsENS_8BandArgsE"


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_the_step_units_hold_the_step_kernels_of_their_lists_without_scratch_or_hazard(listed):  # noqa: F811
    import mfma_hazard_lint as lint
    srcs = [f"sage_attn_d{D}_{u}.hip" for u in STEP_UNITS for D in (128, 64)]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert all(s in re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split() for s in srcs)
    # the lint's new tuple names them and is disjoint from the others, whose contents stand
    assert lint.UNITS_PAGED_STEP == tuple(srcs)
    rest = (lint.UNITS + lint.UNITS_PAIR + lint.UNITS_WINDOW + lint.UNITS_PACKED_BR + lint.UNITS_PACKED_WINDOW + lint.UNITS_GQA_PACK + lint.UNITS_KV_SPLIT +
            lint.UNITS_PAGED + lint.UNITS_PAGED_SPLIT + lint.UNITS_PAGED_RAGGED)
    assert not set(srcs) & set(rest) and len(rest) == 32
    assert lint.UNITS_PAGED_RAGGED == ("sage_attn_d128_f8pr.hip", "sage_attn_d64_f8pr.hip")
    with ThreadPoolExecutor(max_workers=2 * len(srcs)) as ex:
        reports = ex.map(tbr._resource_report, srcs)
        lints = ex.map(lambda u: lint.lint(lint.listing(u)), srcs)
        reports, lints = dict(zip(srcs, reports)), dict(zip(srcs, lints))
    for u, units in STEP_UNITS.items():
        for D in (128, 64):
            src = f"sage_attn_d{D}_{u}.hip"
            rep = reports[src]
            every = {}
            for unit in units:
                every.update(listed[(unit, D)])
            # the QSTART forms of the lists: all four of the ragged units' forms, four of the packed-group list's eight
            want = {w: waves for w, waves in every.items() if kf.unpack(w)["qstart"]}
            assert len(want) == 4 and len(every) == (4 if u == "f8pb" else 8)
            assert not [k for k in rep if "sage_attn_kernel" in k or "sage_attn_paged_kernel" in k or "sage_attn_paged_varlen_kernel" in k], \
                "a kernel of another entry in a step unit"
            assert len(rep) == 4, sorted(rep)
            for name, res in rep.items():
                m = re.fullmatch(STEP_NAME, name)
                assert m, name
                word = int(m.group(1))
                f = kf.unpack(word)
                assert word in want and f["D"] == D and f["causal"] and f["qstart"] and f["kvlen"] and f["pv_fp8"] and not f["seed"], (name, f)
                assert bool(f["gpack"]) == (u == "f8pbg") and f["qf"] in (1, 2), (name, f)
                assert res["VGPRs Spill"] == 0 and res["ScratchSize"] == 0 and res.get("SGPRs Spill", 0) == 0, (name, res)
                assert res["Occupancy"] >= want[word] == (3 if D == 64 else 2), (name, res)          # the form's own bound: no two-wave fallback
            assert {int(re.fullmatch(STEP_NAME, k).group(1)) for k in rep} == set(want)
            assert {kf.unpack(w)["window"] for w in want} == {0, 1} and {kf.unpack(w)["qf"] for w in want} == {1, 2}
            findings, n_mfma = lints[src]
            assert n_mfma >= 100 and not findings, (src, n_mfma, findings[:5])
    # the ragged units hold what they held: exactly their four kernels of the parent's entry (the same body, its band switch off)
    for D in (128, 64):
        text = open(os.path.join(CSRC, f"sage_attn_d{D}_f8pr.hip")).read()
        assert "launch_attn_ragged_units" in text and "step" not in text
    form_h = open(os.path.join(CSRC, "sage_attn_form.h")).read()
    assert "X(F8) X(F8F) X(F16) X(F8V) X(F8VB) X(F8VBW) X(F8S) X(F8K) X(F8Q) X(F8W) X(F8G) X(F8KS)\n" in form_h and "FORM_BITS = 18" in form_h
