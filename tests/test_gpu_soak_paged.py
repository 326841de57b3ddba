"""Soak of the six paged units (GPU): ``*_f8p``, ``*_f8pg``, ``*_f8pks``, ``*_f8pr`` and the step call's ``*_f8pb`` / ``*_f8pbg``.

tests/test_gpu_soak_routes.py's scheme -- ``SAGE_SOAK_ITERS`` iterations of two launches alternating between two streams, a competing GEMM every
fourth iteration, every launch ``torch.equal`` to the first, o and lse -- pointed at the units that compile the hand-scheduled pipelined loop
behind a block-table lookup.  Each is register-allocated and scheduled on its own, so a missed hazard would be this unit's alone, and shows as a
launch that differs, not as a wrong number every time.  One call per unit family, on the shared caches of the tile-count sweep
(tests/test_gpu_paged_tile_counts.py: 111 samples -- 233 for the split -- whose work items run 0 .. 3 trips of the six-body loop with every
remainder), at D 128 on pages of 64 keys and at D 64 on pages of 256.

The offsets, the packed prefix arrays' derived tensors, the split's workspace and the outputs come from ``torch.empty``: every case also runs
test_gpu_soak.py's allocator check -- the caching allocator's free blocks full of NaN patterns, then of 0x5A bytes, the same bits.

A differing launch is a finding, not flakiness: the message says how many launches differ and where the last one does.
"""
import os

import pytest
import torch

import loop_plan as lp
import test_gpu_paged_tile_counts as tc
from test_gpu_soak_routes import _where

pytestmark = pytest.mark.gpu
_SOAK_ITERS = int(os.environ.get("SAGE_SOAK_ITERS", "100"))      # two launches per iteration, as test_gpu_soak.py

if torch.cuda.is_available():
    from sageattention_amd import _cabi
    from sageattention_amd.kv_cache import sageattn_kvcache
    from sageattention_amd.paged_kv_split import sageattn_kvcache_split
    from sageattention_amd.paged_kv_step import sageattn_kvcache_step
    from sageattention_amd.paged_kv_varlen import sageattn_kvcache_varlen
    DEV = torch.device("cuda:0")

NAMES = ("f8p_window", "f8pg_offsets", "f8pks_s3_packed", "f8pr_rotation", "step_rotation_window")
CASES = [(name, D) for name in NAMES for D in (128, 64)]
IDS = [f"{name}-d{D}" for name, D in CASES]
HQ = 4 * tc.HKV


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()
    yield
    for f in (tc._content, tc._caches, tc._q, tc._rows):
        f.cache_clear()
    torch.cuda.empty_cache()


def _make(name, D):
    """The call of a case, as a function without arguments that returns (o, lse)."""
    dt, page_size = (tc.BF16, 64) if D == 128 else (tc.F16, 256)
    if name == "f8pks_s3_packed":                     # pages of 256 keys: chunk 1 starts inside a page
        _, c = tc._caches(D, dt, page_size, "split")
        q, s = tc._q(D, dt, 5 * tc.HKV, 16, "split"), tc._starts("split")
        return lambda: sageattn_kvcache_split(q, c, 3, pack_gqa=True, is_causal=True, q_start=s, return_lse=True)
    _, c = tc._caches(D, dt, page_size, "main")
    W = lp.paged_window_anchor()[0]
    if name == "f8p_window":
        q, s = tc._q(D, dt, HQ, lp.LQ, "main"), tc._starts("main")
        return lambda: sageattn_kvcache(q, c, is_causal=True, q_start=s, window_size=(W - 1, 0), return_lse=True)
    if name == "f8pg_offsets":
        q, s = tc._q(D, dt, HQ, 16, "main"), tc._starts("main")
        return lambda: sageattn_kvcache(q, c, is_causal=True, q_start=s, pack_gqa=True, return_lse=True)
    rotation = lp.paged_ragged_anchor("two0")[0]
    counts, q, kw = tc._ragged_operands(D, dt, HQ, rotation, W if name == "step_rotation_window" else 0, False)
    cu = tc._ints(tc._cu(counts))
    fn = sageattn_kvcache_step if name.startswith("step") else sageattn_kvcache_varlen
    return lambda: fn(q, c, cu, tc.MAX_ROWS, return_lse=True, **kw)


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


@pytest.mark.parametrize("case", CASES, ids=IDS)
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
