"""Soak of the FP8-PV units behind ``kv_lens``, ``q_start``, ``window_size``, ``pack_gqa``, the packed FP8-PV launches and the exact split (GPU).

test_gpu_soak.py's scheme -- ``SAGE_SOAK_ITERS`` iterations of two launches alternating between two streams, a competing GEMM every fourth
iteration, every launch ``torch.equal`` to the first, o and lse -- pointed at the compilation units that file does not reach: ``*_f8k``,
``*_f8q``, ``*_f8w``, ``*_f8g`` (four waves of four different heads over one K / V ring: no repeated-launch test until now), ``*_f8v``,
``*_f8vb``, ``*_f8vbw`` and ``*_f8s``.  Each includes the hand-scheduled pipelined loop and is register-allocated and scheduled on its own,
so a missed hazard or a race would be this unit's alone.  One case per family at D = 128 and D = 64, at shapes no larger than that file's.

Three routes (``pack_gqa`` with a window, the packed window, the exact split) also run test_gpu_soak.py's allocator check: their offsets,
plans, chunk maxima and FP32 partials come from ``torch.empty``, and the result must not depend on what those blocks held.

A differing launch is a finding, not flakiness: the message says how many launches differ and where the last one does.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
_SOAK_ITERS = int(os.environ.get("SAGE_SOAK_ITERS", "100"))      # two launches per iteration, as test_gpu_soak.py

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi
    DEV = torch.device("cuda:0")

F16, BF16 = torch.float16, torch.bfloat16
VARLEN_LENS = (2048, 1, 640, 129, 3000, 64, 1500, 777)           # test_gpu_soak.py::test_varlen_200_launches_on_two_streams_are_bit_identical


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _ints(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _dense(B, Hq, Hkv, Lq, Lk, D, dt, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Hq, Lq, D, generator=g).to(dt).to(DEV)
    k = (torch.randn(B, Hkv, Lk, D, generator=g) + torch.randn(1, Hkv, 1, D, generator=g)).to(dt).to(DEV)
    v = torch.randn(B, Hkv, Lk, D, generator=g).to(dt).to(DEV)
    return q, k, v


def _spread(B, L):
    """B lengths spread over [1, L]: the full length, a lone key, and ragged ones between."""
    return [L, 1] + [1 + (L - 1) * i // (B - 1) + 37 * (i & 1) for i in range(1, B - 1)]


def _make(name, D):
    """The call of a case, as a function without arguments that returns (o, lse)."""
    dt = BF16 if D == 128 else F16
    fp8 = sa.sageattn_qk_int8_pv_fp8_cuda
    if name in ("kv_lens_noncausal", "kv_lens_causal", "q_start_unaligned", "window_300_bottom_right"):
        q, k, v = _dense(4, 8, 4, 2048, 2048, D, dt, 11 + len(name))
        lens = _ints(_spread(4, 2048))
        kw = {"kv_lens_noncausal": dict(is_causal=False), "kv_lens_causal": dict(is_causal=True),
              "q_start_unaligned": dict(is_causal=True, q_start=_ints([5, -1000, 333, 1091])),
              "window_300_bottom_right": dict(is_causal=True, causal_align="bottom_right", window_size=(300, 0))}[name]
        return lambda: fp8(q, k, v, kv_lens=lens, return_lse=True, **kw)
    if name.startswith("pack_gqa"):
        lq = 1 if "lq1" in name else 16
        q, k, v = _dense(8, 32, 8, lq, 2048, D, dt, 13 + len(name))
        lens = _ints(_spread(8, 2048))
        kw = dict(window_size=(300, 0)) if "window" in name else {}
        return lambda: fp8(q, k, v, kv_lens=lens, is_causal=True, causal_align="bottom_right", pack_gqa=True, return_lse=True, **kw)
    if name.startswith("varlen"):
        total = sum(VARLEN_LENS)
        g = torch.Generator().manual_seed(17 + len(name))
        q = torch.randn(total, 8, D, generator=g).to(dt).to(DEV)
        k = (torch.randn(total, 4, D, generator=g) + torch.randn(1, 4, D, generator=g)).to(dt).to(DEV)
        v = torch.randn(total, 4, D, generator=g).to(dt).to(DEV)
        cu = torch.nn.functional.pad(torch.tensor(VARLEN_LENS).cumsum(0), (1, 0)).to(torch.int32).to(DEV)
        kw = {"varlen_plain": dict(is_causal=False), "varlen_bottom_right": dict(is_causal=True, causal_align="bottom_right"),
              "varlen_bottom_right_window": dict(is_causal=True, causal_align="bottom_right", window_size=(300, 0))}[name]
        return lambda: sa.sageattn_qk_int8_pv_fp8_varlen(q, k, v, cu, cu, max(VARLEN_LENS), max(VARLEN_LENS), return_lse=True, **kw)
    assert name == "split_exact_ragged"
    q, k, v = _dense(1, 8, 8, 128, 4096 + 5, D, dt, 19)
    return lambda: fp8(q, k, v, is_causal=False, split_kv_exact=True, split_kv=4, return_lse=True)      # (4101 keys: four chunks of 16 whole tiles and a ragged rest)


NAMES = ("kv_lens_noncausal", "kv_lens_causal", "q_start_unaligned", "window_300_bottom_right", "pack_gqa_lq1", "pack_gqa_lq16",
         "pack_gqa_lq16_window", "varlen_plain", "varlen_bottom_right", "varlen_bottom_right_window", "split_exact_ragged")
CASES = [(name, D) for name in NAMES for D in (128, 64)]
IDS = [f"{name}-d{D}" for name, D in CASES]


def _where(got, want):
    """Which elements of (o, lse) differ: counts and the first index of each."""
    out = []
    for what, a, b in zip(("o", "lse"), got, want):
        ne = a != b
        if bool(ne.any()):
            out.append(f"{what}: {int(ne.sum())} of {a.numel()} differ, first at {tuple(int(i) for i in ne.nonzero()[0])}")
    return "; ".join(out)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_200_launches_on_two_streams_are_bit_identical(case):
    name, D = case
    fn = _make(name, D)
    first = fn()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(first[0].float()).any()) and not bool(torch.isnan(first[1]).any())
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device=DEV, dtype=torch.bfloat16)
    bad, last = 0, ""
    for i in range(_SOAK_ITERS):
        with torch.cuda.stream(side):
            if i % 4 == 0:
                (a @ a).sum()                      # a competing kernel on the other stream
            r2 = fn()
        r1 = fn()
        torch.cuda.synchronize()
        for r in (r1, r2):
            if not (torch.equal(r[0], first[0]) and torch.equal(r[1], first[1])):
                bad += 1
                last = f"iteration {i}: {_where(r, first)}"
    assert bad == 0, f"{name} d{D}: {bad} of {2 * _SOAK_ITERS} launches differ from the first ({last})"


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("pack_gqa_lq16_window", "varlen_bottom_right_window", "split_exact_ragged")],
                         ids=[i for c, i in zip(CASES, IDS) if c[0] in ("pack_gqa_lq16_window", "varlen_bottom_right_window", "split_exact_ragged")])
def test_results_do_not_depend_on_what_the_allocator_hands_out(case):
    """test_gpu_soak.py's check: once with the caching allocator's free blocks full of NaN patterns, once full of 0x5A bytes -- the same bits as
    a call on fresh memory."""
    name, D = case
    fn = _make(name, D)
    want = tuple(t.clone() for t in fn())
    torch.cuda.synchronize()
    for fill in (float("nan"), None):
        torch.cuda.empty_cache()
        junk = [torch.empty(1 << 24, device=DEV) for _ in range(16)]          # 1 GiB of blocks the next allocations are cut from
        for j in junk:
            if fill is None:
                j.view(torch.uint8).fill_(0x5A)
            else:
                j.fill_(fill)
        del junk
        got = fn()
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), \
            f"{name} d{D}: the result depends on stale memory ({'NaN' if fill is not None else '0x5A'} fill): {_where(got, want)}"
