"""Soak of the kv_lens split (``num_splits=``: pass 1, the ``*_f8ks`` units, the merge) and of the appendable KV cache's kernels (GPU).

test_gpu_soak_routes.py's scheme unchanged -- ``SAGE_SOAK_ITERS`` iterations of two launches alternating between two streams, a competing GEMM
every fourth iteration, every launch ``torch.equal`` to the first, o and lse, that file's ``_where`` message on a difference -- pointed at the
units that file does not reach.  Each ``f8ks`` unit includes the hand-scheduled pipelined loop and is register-allocated and scheduled on its
own; the split's three launches pass chunk maxima and FP32 partials through a workspace from ``torch.empty``; the cache's two append kernels
re-form an open block in place.  One case per family at D = 128 and D = 64, at shapes no larger than that file's.

The KV-cache step starts every iteration from a fresh ``from_prefill`` of the same content on that iteration's stream, appends one row and
attends (``pack_gqa=True``, bottom-right); o, lse and the cache's bytes wherever its content defines them -- rows < len, the scale slots and V
tiles of blocks that hold rows, the tails of the open block, lens -- equal the first iteration's.

The three ``num_splits`` cases also run that file's allocator check: the result must not depend on what ``torch.empty`` hands back for the
workspace.  Blocks of the workspace's own size are filled and freed in front of the call (a decode call's workspace is below the caching
allocator's small-allocation threshold and is never cut from that file's 64 MiB blocks), and the test asserts that the workspace the call got
lies inside filled memory.

A differing launch is a finding, not flakiness: the message says how many launches differ and where the last one does.
"""
import pytest
import torch

from test_gpu_soak_routes import _SOAK_ITERS, _dense, _ints, _spread, _where

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, ops
    from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
    DEV = torch.device("cuda:0")

F16, BF16 = torch.float16, torch.bfloat16
BR = dict(is_causal=True, causal_align="bottom_right")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _make(name, D):
    """The call of a ``num_splits`` case, as a function without arguments that returns (o, lse)."""
    dt = BF16 if D == 128 else F16
    fp8 = sa.sageattn_qk_int8_pv_fp8_cuda
    if name == "split4_packed_bottom_right_lq1":
        q, k, v = _dense(8, 32, 8, 1, 2048, D, dt, 23)
        lens = _ints(_spread(8, 2048))
        return lambda: fp8(q, k, v, kv_lens=lens, pack_gqa=True, num_splits=4, return_lse=True, **BR)
    if name == "split4_noncausal_lq33":
        q, k, v = _dense(4, 8, 4, 33, 2048, D, dt, 29)
        lens = _ints(_spread(4, 2048))
        return lambda: fp8(q, k, v, kv_lens=lens, is_causal=False, pack_gqa=False, num_splits=4, return_lse=True)
    assert name == "split7_q_start_unaligned_lq128"
    q, k, v = _dense(4, 8, 4, 128, 2048, D, dt, 31)
    lens = _ints(_spread(4, 2048))
    return lambda: fp8(q, k, v, kv_lens=lens, is_causal=True, q_start=_ints([1900, -100, 333, 1091]), pack_gqa=False, num_splits=7, return_lse=True)


NAMES = ("split4_packed_bottom_right_lq1", "split4_noncausal_lq33", "split7_q_start_unaligned_lq128")
CASES = [(name, D) for name in NAMES for D in (128, 64)]
IDS = [f"{name}-d{D}" for name, D in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_200_split_launches_on_two_streams_are_bit_identical(case):
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


# (B, Hq, Lq, S) of the cases above: what the split workspace is sized from
SHAPES = {"split4_packed_bottom_right_lq1": (8, 32, 1, 4), "split4_noncausal_lq33": (4, 8, 33, 4), "split7_q_start_unaligned_lq128": (4, 8, 128, 7)}
WS_JUNK = 48                              # blocks of the workspace's size filled and freed in front of the call


def _ranges(tensors):
    """The address ranges of ``tensors``, adjacent ones merged (freed neighbours coalesce in the caching allocator)."""
    out = []
    for a, b in sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in tensors):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_split_results_do_not_depend_on_what_the_allocator_hands_out(monkeypatch, case):
    """test_gpu_soak_routes.py's check on the split workspace (chunk maxima, FP32 partials, per-chunk LSE -- ONE ``torch.empty`` of
    ``kv_split_ws_bytes``): once full of NaN patterns, once full of 0x5A bytes -- the same bits as a call on fresh memory.  That file's 64 MiB
    blocks alone would miss the decode case, whose workspace (0.5 MiB at D = 128) the caching allocator serves from its small pool: so blocks
    of exactly the workspace's size are filled and freed too, with no ``empty_cache()`` behind them, and the workspace the call really got
    must lie inside memory that was filled."""
    name, D = case
    B, Hq, Lq, S = SHAPES[name]
    ws_bytes = _cabi.kv_split_ws_bytes(B, Hq, Lq, D, S)
    fn = _make(name, D)
    want = tuple(t.clone() for t in fn())
    torch.cuda.synchronize()
    seen = []
    real = ops.attn_attr

    def spy(*a, **kw):
        ws = kw.get("split_ws")
        if ws is not None:
            seen.append((ws.data_ptr(), ws.numel() * ws.element_size()))
        return real(*a, **kw)
    monkeypatch.setattr(ops, "attn_attr", spy)
    for fill in (float("nan"), None):
        torch.cuda.empty_cache()
        junk = [torch.empty(1 << 24, device=DEV) for _ in range(16)]          # 1 GiB of blocks the next large allocations are cut from
        junk += [torch.empty(ws_bytes // 4, device=DEV) for _ in range(WS_JUNK)]      # ... and blocks of the workspace's own size
        for j in junk:
            if fill is None:
                j.view(torch.uint8).fill_(0x5A)
            else:
                j.fill_(fill)
        torch.cuda.synchronize()
        filled = _ranges(junk)
        del junk, j
        del seen[:]
        got = fn()
        torch.cuda.synchronize()
        assert len(seen) == 1 and seen[0][1] == ws_bytes, (seen, ws_bytes)
        p0, p1 = seen[0][0], seen[0][0] + ws_bytes
        inside = any(a <= p0 and p1 <= b for a, b in filled)
        print(f"{name} d{D} {'NaN' if fill is not None else '0x5A'}: workspace of {ws_bytes} bytes at {p0:#x}, inside filled memory: {inside}")
        assert inside, f"{name} d{D}: the workspace ({ws_bytes} bytes at {p0:#x}) was not cut from the filled blocks: the check would prove nothing"
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), \
            f"{name} d{D}: the result depends on stale memory ({'NaN' if fill is not None else '0x5A'} fill): {_where(got, want)}"


# ---------------------------------------------------------------------------------------------- the KV-cache step
CACHE_B, CACHE_HQ, CACHE_HKV, CACHE_CAP = 8, 32, 8, 2048


def _parts(cache, lens):
    """(name, tensor) of the cache's bytes wherever its content defines them: v_scale and lens whole; per sample the rows < len, the scale slots
    and V tiles of blocks that hold rows, the tails of the open block."""
    out = [("v_scale", cache.v_scale), ("lens", cache.lens)]
    for b, n in enumerate(lens):
        nb, r = (n + 63) // 64, n % 64
        out += [(f"sample {b} k_int8", cache.k_int8[b, :, :n]), (f"sample {b} k_scale", cache.k_scale[b, :, :nb * 4]),
                (f"sample {b} v_image", cache.v_image[b, :, :nb]), (f"sample {b} k_tail", cache.k_tail[b, :, :r]), (f"sample {b} v_tail", cache.v_tail[b, :, :r])]
    return out


def _defined(cache, lens):
    """Those bytes as one tensor."""
    return torch.cat([t.reshape(-1).view(torch.uint8) for _, t in _parts(cache, lens)])


@pytest.mark.parametrize("D", (128, 64))
def test_200_cache_steps_on_two_streams_are_bit_identical(D):
    dt = BF16 if D == 128 else F16
    q, k, v = _dense(CACHE_B, CACHE_HQ, CACHE_HKV, 1, CACHE_CAP, D, dt, 37)
    # prefill lengths spread over the capacity: a lone key, an open block one row short of its end (63 -> 64), a block end (64 -> 65)
    have = [n - 1 for n in _spread(CACHE_B, CACHE_CAP - 1)[:CACHE_B - 2]] + [63, 64]
    have[1] = 1
    lens0 = _ints(have)
    rows = torch.stack([k[b, :, n:n + 1] for b, n in enumerate(have)]), torch.stack([v[b, :, n:n + 1] for b, n in enumerate(have)])
    after = [n + 1 for n in have]

    def step():
        cache = QuantizedKVCache.from_prefill(k, v, CACHE_CAP, kv_lens=lens0)
        cache.append(*rows)
        o, lse = sageattn_kvcache(q, cache, pack_gqa=True, return_lse=True, **BR)
        return o, lse, _defined(cache, after), cache

    first = step()
    torch.cuda.synchronize()
    assert first[3].lens.tolist() == after
    assert not bool(torch.isnan(first[0].float()).any()) and bool(torch.isfinite(first[1]).all())
    first_parts = [(name, t.clone()) for name, t in _parts(first[3], after)]
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device=DEV, dtype=torch.bfloat16)
    bad, last = 0, ""
    for i in range(_SOAK_ITERS):
        with torch.cuda.stream(side):
            if i % 4 == 0:
                (a @ a).sum()                      # a competing kernel on the other stream
            r2 = step()
        r1 = step()
        torch.cuda.synchronize()
        for r in (r1, r2):
            if not (torch.equal(r[0], first[0]) and torch.equal(r[1], first[1]) and torch.equal(r[2], first[2])):
                bad += 1
                parts = [name for (name, x), (_, y) in zip(_parts(r[3], after), first_parts) if not torch.equal(x, y)]
                last = f"iteration {i}: {_where(r[:2], first[:2]) or 'o and lse equal'}; cache parts that differ: {parts[:6]}"
    assert bad == 0, f"kv cache step d{D}: {bad} of {2 * _SOAK_ITERS} steps differ from the first ({last})"
