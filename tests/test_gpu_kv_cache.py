"""GPU: the appendable quantised KV cache (``sageattention_amd.kv_cache``, ``sage_kvcache_append``).

Two defining properties, both bit equalities:
  A  a cache seeded with the statistics of its final content holds, whatever the schedule of appends, byte for byte what the length-aware
     pre-pass produces from that content (``per_thread_int8_k_kvlens`` / ``per_channel_fp8_kvlens``), and nothing outside it is written;
  B  ``sageattn_kvcache`` on such a cache returns bit for bit the ``o`` and ``lse`` of ``sageattn_qk_int8_pv_fp8_cuda(q, k, v, kv_lens=...)``.
Then the cache as it is used -- statistics frozen at prefill time, with head-room -- against FP64 attention, relative to the one-shot call's
own error; saturation beyond the frozen range; the capacity clamp under guarded memory; capture into a graph.
Then the cache as a decode loop drives it: property A and B after EVERY append of seeded random schedules (an open block that is wrong until a
later append re-forms it shows at once); rows appended as a caller holds them -- slices of larger tensors, no copy made here; a used cache
seeded again.

Shapes -- the smallest that can still go wrong: B 4, Hq 8, Hkv 2, capacity 320 (five 64-key blocks) and the final lengths
  257  four whole blocks and one row         64  exactly one block (the open block is the next, empty one)
  130  two blocks and a ragged one           0   a sample that never gets a row
Every cache tensor is filled with a poison byte before the first append, and the rows of ``k_new`` / ``v_new`` at or behind ``new_lens[b]``
hold NaN bit patterns: a row read that should not be shows in the bytes.
"""
import functools

import numpy as np
import pytest
import torch

import util
from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, quant as sq
    from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
    DEV = torch.device("cuda:0")

B, HQ, HKV, CAP = 4, 8, 2, 320
FINAL = (257, 64, 130, 0)
POISON = 0x5A
F16, BF16 = torch.float16, torch.bfloat16
CASES = [(64, F16, "HND"), (64, BF16, "NHD"), (128, F16, "NHD"), (128, BF16, "HND")]
CASE_IDS = [f"d{D}-{'f16' if dt == F16 else 'bf16'}-{lay}" for D, dt, lay in CASES]

# a schedule: steps of (T, rows each sample takes); every one ends at FINAL.  Counts outside [0, T] are clamped on the device.
SCHEDULES = {
    "one": [(257, FINAL)],
    "rows": [(1, tuple(int(i < n) for n in FINAL)) for i in range(257)],
    "mixed": [(63, (63 + 7, 0, 63, -5)), (1, (1, 1, 0, 0)), (1, (1, 0, 1, 0)), (63, (63, 63, 2, 0)), (2, (2, 0, 2, -1)), (64, (64, 0, 62, 0)),
              (63, (63, 0, 0, 0))],
    "cross": [(127, (127, 64, 0, 0)), (130, (130, 0, 130, 0))],      # one call whose rows cross two (sample 2) and three (sample 0) block ends
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _lay(t, layout):
    return t if layout == "HND" else t.transpose(1, 2).contiguous()


def _hnd(t, layout):
    return t if layout == "HND" else t.transpose(1, 2)


def _ints(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _u8(t):
    return t.contiguous().view(torch.uint8)


@functools.lru_cache(maxsize=None)
def _content(D, dt, layout):
    """k, v ``[B, HKV, CAP, D]`` in ``layout`` (random rows behind the final lengths too), and what the pre-pass makes of their first FINAL
    rows: computed once, never modified."""
    g = torch.Generator().manual_seed(11 + D)
    k = (torch.randn(B, HKV, CAP, D, generator=g) + 1.5 * torch.randn(1, HKV, 1, D, generator=g)).to(dt)
    v = (torch.randn(B, HKV, CAP, D, generator=g) * (0.25 + torch.rand(1, HKV, 1, D, generator=g))).to(dt)
    k, v = _lay(k.to(DEV), layout), _lay(v.to(DEV), layout)
    lens = _ints(FINAL)
    km = sq.channel_mean_kvlens(k, lens, layout)
    k_int8, k_scale = sq.per_thread_int8_k_kvlens(k, km, lens, layout)
    v_image, v_scale = sq.per_channel_fp8_kvlens(v, lens, layout)
    valid = (torch.arange(CAP, device=DEV)[None, :] < lens[:, None]).view(B, 1, CAP, 1)
    v_amax = torch.where(valid, _hnd(v, layout).abs().float(), 0.0).amax(dim=2)          # exact: the fp32 abs-max of the valid rows
    torch.cuda.synchronize()
    return k, v, km, v_amax, _hnd(k_int8, layout).contiguous(), k_scale, v_image, v_scale


def _poisoned_cache(D, dt):
    c = QuantizedKVCache.allocate(B, HKV, CAP, D, dt, DEV)
    for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail, c.lens):
        t.view(torch.uint8).fill_(POISON)
    return c


def _rows(x, layout, offsets, counts, T):
    """``[B, HKV, T, D]`` in ``layout``: sample b's first ``clamp(counts[b], 0, T)`` rows are ``x[b, :, offsets[b]:...]`` (as far as ``x`` has
    rows), the rest NaN bits."""
    xh = _hnd(x, layout)
    out = torch.full((B, HKV, T, xh.shape[-1]), -1, dtype=torch.int16, device=DEV).view(x.dtype)        # 0xFFFF: NaN as fp16 and as bf16
    for b in range(B):
        n = max(0, min(int(counts[b]), T, xh.shape[2] - offsets[b]))
        out[b, :, :n] = xh[b, :, offsets[b]:offsets[b] + n]
    return _lay(out, layout)


def _fill(cache, k, v, layout, schedule):
    have = [0] * B
    for T, counts in schedule:
        cache.append(_rows(k, layout, have, counts, T), _rows(v, layout, have, counts, T), _ints(counts), layout)
        have = [h + max(0, min(int(c), T)) for h, c in zip(have, counts)]
    return have


@functools.lru_cache(maxsize=None)
def _filled(D, dt, layout, name):
    """The poisoned cache seeded with the final content's statistics and filled by schedule ``name``: built once, shared, never modified."""
    k, v, km, v_amax = _content(D, dt, layout)[:4]
    c = _poisoned_cache(D, dt)
    c.seed(km, v_amax)
    assert tuple(_fill(c, k, v, layout, SCHEDULES[name])) == FINAL
    torch.cuda.synchronize()
    return c


@pytest.mark.parametrize("name", list(SCHEDULES))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_bytes_are_the_prepass_bytes(case, name):
    """Property A.  INT8 rows < len, the scale slots of blocks that hold rows, the V tiles that hold rows (zero tails included), v_scale and
    lens equal the pre-pass's byte for byte; everything else still holds the poison; the tails hold the open block's raw rows."""
    D, dt, layout = case
    k, v, km, v_amax, ref_k, ref_ks, ref_vi, ref_vs = _content(*case)
    c = _filled(D, dt, layout, name)
    assert c.lens.tolist() == list(FINAL)
    assert torch.equal(c.v_scale.view(torch.int32), ref_vs.view(torch.int32)), "v_scale"
    assert torch.equal(c.k_mean, km) and torch.equal(c.v_amax, v_amax)
    kh, vh = _hnd(k, layout), _hnd(v, layout)
    for b, n in enumerate(FINAL):
        nb = (n + 63) // 64
        assert torch.equal(c.k_int8[b, :, :n], ref_k[b, :, :n]), f"sample {b}: INT8 rows differ in {int((c.k_int8[b, :, :n] != ref_k[b, :, :n]).sum())} bytes"
        assert bool((_u8(c.k_int8[b, :, n:]) == POISON).all()), f"sample {b}: INT8 rows behind {n} written"
        assert torch.equal(c.k_scale[b, :, :nb * 4].view(torch.int32), ref_ks[b, :, :nb * 4].view(torch.int32)), f"sample {b}: k scales"
        assert bool((_u8(c.k_scale[b, :, nb * 4:]) == POISON).all()), f"sample {b}: scale slots behind block {nb} written"
        assert torch.equal(c.v_image[b, :, :nb], ref_vi[b, :, :nb]), f"sample {b}: V image differs in {int((c.v_image[b, :, :nb] != ref_vi[b, :, :nb]).sum())} bytes"
        assert bool((c.v_image[b, :, nb:] == POISON).all()), f"sample {b}: V tiles behind {nb} written"
        r = n % 64
        assert torch.equal(c.k_tail[b, :, :r], kh[b, :, n - r:n]) and torch.equal(c.v_tail[b, :, :r], vh[b, :, n - r:n]), f"sample {b}: tails"
    assert bool((_u8(c.k_tail[3]) == POISON).all()) and bool((_u8(c.v_tail[3]) == POISON).all())       # the sample without rows
    if name == "one":                 # (the other schedules leave a finished block's rows in the tails)
        for b, n in enumerate(FINAL):
            assert bool((_u8(c.k_tail[b, :, n % 64:]) == POISON).all()) and bool((_u8(c.v_tail[b, :, n % 64:]) == POISON).all())


# (Lq, keywords): every mask kind, the window, the packed launch (Lq <= 32), both ways to ask for a split
VARIANTS = [
    (40, dict()),
    (40, dict(is_causal=True)),
    (40, dict(is_causal=True, causal_align="bottom_right")),
    (40, dict(is_causal=True, causal_align="bottom_right", window_size=(70, 0))),
    (40, dict(num_splits=2)),
    (16, dict(pack_gqa=True)),
    (16, dict(is_causal=True, pack_gqa=True)),
    (16, dict(is_causal=True, causal_align="bottom_right", pack_gqa=True, window_size=(70, 0))),
    (16, dict(is_causal=True, causal_align="bottom_right", num_splits=2)),
    (16, dict(num_splits="auto", pack_gqa=True)),
    (1, dict()),
    (1, dict(is_causal=True, causal_align="bottom_right", pack_gqa=True)),
    (1, dict(is_causal=True, causal_align="bottom_right", pack_gqa=True, num_splits=2)),
    (1, dict(is_causal=True, causal_align="bottom_right", window_size=(70, 0))),
    (1, dict(num_splits="auto")),
]
VARIANT_IDS = [f"lq{lq}-" + ("-".join(f"{k_}={v_}" for k_, v_ in kw.items()) or "plain").replace(" ", "") for lq, kw in VARIANTS]


def _q(D, dt, layout, lq, seed=5):
    g = torch.Generator().manual_seed(seed + D + lq)
    return _lay(torch.randn(B, HQ, lq, D, generator=g).to(dt).to(DEV), layout)


@pytest.mark.parametrize("variant", range(len(VARIANTS)), ids=VARIANT_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_attention_is_the_one_shot_call(case, variant):
    """Property B, on the caches of every schedule: o and lse bit for bit; the empty sample gives o = 0, lse = -inf."""
    D, dt, layout = case
    lq, kw = VARIANTS[variant]
    k, v = _content(*case)[:2]
    q = _q(D, dt, layout, lq)
    o_ref, lse_ref = sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, tensor_layout=layout, kv_lens=_ints(FINAL), return_lse=True, **kw)
    for name in SCHEDULES:
        o, lse = sageattn_kvcache(q, _filled(D, dt, layout, name), tensor_layout=layout, return_lse=True, **kw)
        assert o.shape == q.shape and o.dtype == dt and lse.shape == (B, HQ, lq)
        assert torch.equal(o, o_ref), f"{name}: o differs in {int((o != o_ref).sum())} of {o.numel()} elements"
        assert torch.equal(lse, lse_ref), f"{name}: lse differs in {int((lse != lse_ref).sum())} of {lse.numel()} rows"
        assert bool((o[3] == 0).all()) and bool((lse[3] == float("-inf")).all())
        assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse[:3]).any())
    o_only = sageattn_kvcache(q, _filled(D, dt, layout, "one"), tensor_layout=layout, **kw)
    assert torch.equal(o_only, o_ref)


# ---- frozen statistics as a caller uses them ---------------------------------------------------------------------------------------
# The cache is seeded from the first 192 rows (k_mean of those rows, v_amax = 2 x their abs-max) and grows by 65 single rows; the one-shot call
# forms its statistics over all 257.  Both errors are rel-RMS of o against FP64 softmax attention on the same fp16 / bf16 inputs.  The argument
#  says the ratio is near 1: any k_mean is exact, and head-room on v_amax moves e4m3's exponent, not its precision.
# Measured on an MI355X, seeds 0 .. 11 of each case below (24 draws; err_oneshot 3.4e-2 .. 3.7e-2): ratios 0.989 .. 1.011, FROZEN_MEASURED.
# FROZEN_C = 1.25 x the largest ratio, rounded up to one decimal: 1.25 x 1.0112 = 1.264 -> 1.3.
FROZEN_CASES = [(128, BF16, "HND"), (64, F16, "NHD")]
FROZEN_SEEDS = range(8)
FROZEN_MEASURED = (0.9892, 1.0112)      # (smallest, largest) measured ratio err_cache / err_oneshot
FROZEN_C = 1.3


def _f64_attention(q, k, v):
    """softmax(q k^T / sqrt(D)) v in FP64, HND operands, GQA by repetition"""
    qf, kf, vf = q.double(), k.double(), v.double()
    g = qf.shape[1] // kf.shape[1]
    kf, vf = kf.repeat_interleave(g, 1), vf.repeat_interleave(g, 1)
    s = qf @ kf.transpose(-1, -2) * qf.shape[-1] ** -0.5
    return torch.softmax(s, dim=-1) @ vf


def frozen_errors(D, dt, layout, seed):
    """(err_cache, err_oneshot) of one draw: 192 prefill rows, 65 single-row appends, 16 query rows that see all 257 keys."""
    n0, n1, lq = 192, 257, 16
    g = torch.Generator().manual_seed(1000 + seed)
    k = (torch.randn(B, HKV, n1, D, generator=g) + 2.0 * torch.randn(1, HKV, 1, D, generator=g)).to(dt).to(DEV)      # a per-channel offset: smoothing matters
    v = torch.randn(B, HKV, n1, D, generator=g).to(dt).to(DEV)
    q = torch.randn(B, HQ, lq, D, generator=g).to(dt).to(DEV)
    ref = _f64_attention(q, k, v)
    kl, vl, ql = _lay(k, layout), _lay(v, layout), _lay(q, layout)
    seq = 2 if layout == "HND" else 1
    cache = QuantizedKVCache.from_prefill(kl.narrow(seq, 0, n0), vl.narrow(seq, 0, n0), CAP, tensor_layout=layout, v_headroom=2.0)
    for i in range(n0, n1):
        cache.append(kl.narrow(seq, i, 1), vl.narrow(seq, i, 1), tensor_layout=layout)
    o_cache = _hnd(sageattn_kvcache(ql, cache, tensor_layout=layout), layout)
    o_shot = _hnd(sa.sageattn_qk_int8_pv_fp8_cuda(ql, kl, vl, tensor_layout=layout, kv_lens=_ints([n1] * B)), layout)
    assert cache.lens.tolist() == [n1] * B
    rel = lambda o: float(((o.double() - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())
    return rel(o_cache), rel(o_shot)


@pytest.mark.parametrize("case", FROZEN_CASES, ids=[f"d{D}-{'f16' if dt == F16 else 'bf16'}-{lay}" for D, dt, lay in FROZEN_CASES])
def test_frozen_statistics_cost_no_accuracy(case):
    for seed in FROZEN_SEEDS:
        err_cache, err_shot = frozen_errors(*case, seed)
        print(f"frozen statistics {case} seed {seed}: err_cache {err_cache:.4e} err_oneshot {err_shot:.4e} ratio {err_cache / err_shot:.3f}")
        assert 0.0 < err_shot < 0.1 and err_cache <= FROZEN_C * err_shot, (seed, err_cache, err_shot)


@pytest.mark.parametrize("case", CASES[2:], ids=CASE_IDS[2:])
def test_values_beyond_the_frozen_range_saturate(case):
    """Appended V rows at 8 x the frozen v_amax give the e4m3 bytes of +-448 (0x7E / 0xFE) in their positions, and a finite output."""
    D, dt, layout = case
    g = torch.Generator().manual_seed(3)
    v_amax = (0.5 + torch.rand(B, HKV, D, generator=g)).to(DEV)
    c = _poisoned_cache(D, dt)
    c.seed(None, v_amax)
    k = _lay(torch.randn(B, HKV, 70, D, generator=g).to(dt).to(DEV), layout)
    sign = torch.where(torch.rand(B, HKV, 70, D, generator=g) < 0.5, -1.0, 1.0).to(DEV)
    big = torch.zeros(B, HKV, 70, 1, dtype=torch.bool, device=DEV)
    big[:, :, 5] = big[:, :, 63] = big[:, :, 64] = big[:, :, 69] = True
    vh = torch.where(big, 8.0 * v_amax[:, :, None, :] * sign, 0.25 * v_amax[:, :, None, :] * sign).to(dt)
    c.append(k, _lay(vh, layout), tensor_layout=layout)
    torch.cuda.synchronize()
    img = util.decode_v_image(c.v_image[:, :, :2].cpu().numpy(), 70, True)          # [B, HKV, 70, D] e4m3 bytes
    want = np.where(sign.cpu().numpy() > 0, 0x7E, 0xFE)
    rows = big[0, 0, :, 0].cpu().numpy()
    assert (img[:, :, rows] == want[:, :, rows]).all()
    assert ((img[:, :, ~rows] & 0x7F) < 0x7E).all() and ((img[:, :, ~rows] & 0x7F) > 0).all()
    o = sageattn_kvcache(_q(D, dt, layout, 16), c, tensor_layout=layout)
    assert bool(torch.isfinite(o.float()).all())


@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=[CASE_IDS[1], CASE_IDS[3]])
def test_capacity_clamps_and_nothing_is_written_past_a_buffer(case, fill):
    """An append that would pass ``capacity`` leaves ``lens == capacity`` and drops the excess; the guard regions behind (and in front of)
    every cache tensor keep their fill, as do the cache's bytes past each sample's rows."""
    D, dt, layout = case
    k, v = _content(*case)[:2]
    full = _ints([CAP] * B)
    km = sq.channel_mean_kvlens(k, full, layout)
    v_amax = _hnd(v, layout).abs().float().amax(dim=2)
    ref_k, ref_ks = sq.per_thread_int8_k_kvlens(k, km, full, layout)
    ref_vi, _ = sq.per_channel_fp8_kvlens(v, full, layout)
    with Fence(fill) as f:
        c = QuantizedKVCache.allocate(B, HKV, CAP, D, dt, DEV)
        assert all(f.owns(t) for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail, c.lens))
        c.seed(km, v_amax)
        have = _fill(c, k, v, layout, [(300, (300, 257, 319, 0))])
        # 100 more rows each: samples 0 .. 2 run into the capacity (20, 63 and 1 rows fit), sample 3 takes all 100
        c.append(_rows(k, layout, have, [100] * B, 100), _rows(v, layout, have, [100] * B, 100), None, layout)
        assert c.lens.tolist() == [CAP, CAP, CAP, 100]
        c.append(_rows(k, layout, [0] * B, [64] * B, 64), _rows(v, layout, [0] * B, [64] * B, 64), _ints([64, 64, 64, 0]), layout)      # a full cache takes nothing
        assert c.lens.tolist() == [CAP, CAP, CAP, 100]
        f.check()
        for b in range(3):
            assert torch.equal(c.k_int8[b], _hnd(ref_k, layout)[b]) and torch.equal(c.k_scale[b].view(torch.int32), ref_ks[b].view(torch.int32))
            assert torch.equal(c.v_image[b], ref_vi[b])
        assert bool((_u8(c.k_int8[3, :, 100:]) == fill).all()) and bool((c.v_image[3, :, 2:] == fill).all()) and bool((_u8(c.k_scale[3, :, 8:]) == fill).all())


def test_append_and_attention_capture_into_a_graph():
    """``append`` + ``sageattn_kvcache`` captured on one stream; three replays with new rows written into the captured inputs are bit-equal to
    the eager sequence, outputs and cache."""
    D, dt, layout = 128, BF16, "HND"
    k, v = _content(D, dt, layout)[:2]
    n0 = 62          # the replays take the open block over a block end: 62 -> 63 -> 65 -> 66 (the middle step appends two rows)

    def fresh():
        return QuantizedKVCache.from_prefill(k[:, :, :n0], v[:, :, :n0], CAP, kv_lens=_ints([n0, n0, 3, 0]), v_headroom=1.5)

    def step(cache, k_in, v_in, n_in, q_in):
        cache.append(k_in, v_in, n_in)
        return sageattn_kvcache(q_in, cache, is_causal=True, causal_align="bottom_right", pack_gqa=True, return_lse=True)

    steps = [(k[:, :, 100 + 2 * i:102 + 2 * i], v[:, :, 100 + 2 * i:102 + 2 * i], _ints(n), _q(D, dt, layout, 1, seed=20 + i))
             for i, n in enumerate([(1, 1, 1, 0), (2, 2, 0, 1), (1, 0, 2, 2)])]
    eager_cache = fresh()
    eager = [tuple(t.clone() for t in step(eager_cache, *s)) for s in steps]

    warm, cache = fresh(), fresh()
    k_in, v_in, n_in, q_in = (t.clone() for t in steps[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(warm, k_in, v_in, n_in, q_in)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o, lse = step(cache, k_in, v_in, n_in, q_in)
    for i, (ks, vs, ns, qs) in enumerate(steps):
        k_in.copy_(ks), v_in.copy_(vs), n_in.copy_(ns), q_in.copy_(qs)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager[i][0]) and torch.equal(lse, eager[i][1]), f"replay {i}"
    assert cache.lens.tolist() == eager_cache.lens.tolist() == [n0 + 4, n0 + 3, 6, 3]
    for name in ("k_int8", "k_scale", "v_image", "v_scale", "k_tail", "v_tail"):
        a, b_ = getattr(cache, name), getattr(eager_cache, name)
        for b, n in enumerate(cache.lens.tolist()):       # (what a cache holds behind its rows is whatever the allocation held)
            nb = (n + 63) // 64
            sl = {"k_int8": (slice(None), slice(0, n)), "k_scale": (slice(None), slice(0, nb * 4)), "v_image": (slice(None), slice(0, nb)),
                  "v_scale": (slice(None),), "k_tail": (slice(None), slice(0, n % 64)), "v_tail": (slice(None), slice(0, n % 64))}[name]
            assert torch.equal(_u8(a[b][sl]), _u8(b_[b][sl])), (name, b)


# ---- after every append ---------------------------------------------------------------------------------------------------------------
# A decode loop attends after every append, so an open block that is wrong until a later append re-forms it is wrong where it matters.  Eight
# seeded random schedules per case; after EVERY step the cache is compared with the pre-pass of the current prefix under the same frozen
# statistics (those of the schedule's final content), and every second step attends.
# (the schedules are ``util.random_append_schedule``; what the eight reach is asserted on the CPU, tests/test_kv_cache_host.py)
STEP_SEEDS = util.APPEND_SCHEDULE_SEEDS


def _check_prefix(c, k, v, km, ref_dec, ref_vs, lens_now, layout, what):
    """The cache against the pre-pass of the current prefix under the frozen statistics.  Returns the reference operands of an attention call
    on that prefix: INT8 K (in ``layout``), its scales, the V image."""
    D = k.shape[-1]
    lens_t = _ints(lens_now)
    ref_k, ref_ks = sq.per_thread_int8_k_kvlens(k, km, lens_t, layout)
    ref_kh = _hnd(ref_k, layout)
    kh, vh = _hnd(k, layout), _hnd(v, layout)
    assert c.lens.tolist() == list(lens_now), what
    now = ref_dec.copy()                                    # the final reference image's e4m3 bytes, key rows >= len zeroed
    for b, n in enumerate(lens_now):
        now[b, :, n:] = 0
    got = util.decode_v_image(c.v_image.cpu().numpy(), CAP, True)
    for b, n in enumerate(lens_now):
        nb, r = (n + 63) // 64, n % 64
        assert torch.equal(c.k_int8[b, :, :n], ref_kh[b, :, :n]), f"{what} sample {b}: INT8 rows differ in {int((c.k_int8[b, :, :n] != ref_kh[b, :, :n]).sum())} bytes"
        assert torch.equal(c.k_scale[b, :, :nb * 4].view(torch.int32), ref_ks[b, :, :nb * 4].view(torch.int32)), f"{what} sample {b}: k scales"
        assert np.array_equal(got[b, :, :nb * 64], now[b, :, :nb * 64]), \
            f"{what} sample {b}: V differs in {int((got[b, :, :nb * 64] != now[b, :, :nb * 64]).sum())} bytes (rows {sorted(set(np.nonzero(got[b, :, :nb * 64] != now[b, :, :nb * 64])[1].tolist()))[:8]})"
        assert torch.equal(c.k_tail[b, :, :r], kh[b, :, n - r:n]) and torch.equal(c.v_tail[b, :, :r], vh[b, :, n - r:n]), f"{what} sample {b}: tails"
        assert bool((_u8(c.k_int8[b, :, n:]) == POISON).all()), f"{what} sample {b}: INT8 rows behind {n} written"
        assert bool((_u8(c.k_scale[b, :, nb * 4:]) == POISON).all()), f"{what} sample {b}: scale slots behind block {nb} written"
        assert bool((c.v_image[b, :, nb:] == POISON).all()), f"{what} sample {b}: V tiles behind {nb} written"
        if n:
            assert torch.equal(c.v_scale[b].view(torch.int32), ref_vs[b].view(torch.int32)), f"{what} sample {b}: v_scale"
    return ref_k, ref_ks, torch.from_numpy(np.ascontiguousarray(util.encode_v_image(now, True))).to(DEV)


@pytest.mark.parametrize("seed", STEP_SEEDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_step_holds_the_prepass_of_its_prefix(case, seed):
    from sageattention_amd import core as sc
    D, dt, layout = case
    k, v = _content(*case)[:2]
    final, steps = util.random_append_schedule(seed, B, CAP)
    lens_f = _ints(final)
    km = sq.channel_mean_kvlens(k, lens_f, layout)
    ref_vi, ref_vs = sq.per_channel_fp8_kvlens(v, lens_f, layout)
    valid = (torch.arange(CAP, device=DEV)[None, :] < lens_f[:, None]).view(B, 1, CAP, 1)
    v_amax = torch.where(valid, _hnd(v, layout).abs().float(), 0.0).amax(dim=2)
    ref_dec = util.decode_v_image(ref_vi.cpu().numpy(), CAP, True)                  # [B, HKV, CAP, D] e4m3 bytes
    c = _poisoned_cache(D, dt)
    c.seed(km, v_amax)
    q = _q(D, dt, layout, 1, seed=40 + seed)
    sm = D ** -0.5
    corr = sc._lse_correction(q, km.unsqueeze(1 if layout == "NHD" else 2), layout)
    have, attended = [0] * B, 0
    print(f"schedule {seed}: final {final}, {len(steps)} steps {[(T, n, kd) for T, n, kd in steps]}")
    for i, (T, counts, kind) in enumerate(steps):
        new_lens = None if kind == "none" else torch.tensor(counts, dtype=torch.int64 if kind == "i64" else torch.int32, device=DEV)
        c.append(_rows(k, layout, have, counts, T), _rows(v, layout, have, counts, T), new_lens, layout)
        have = [h + max(0, min(int(n), T)) for h, n in zip(have, counts)]
        what = f"schedule {seed} step {i} (T {T}, counts {counts}, {kind}) -> {have}"
        ref_k, ref_ks, vi_now = _check_prefix(c, k, v, km, ref_dec, ref_vs, have, layout, what)
        if i & 1 or i == len(steps) - 1:
            lens_t = _ints(have)
            o, lse = sageattn_kvcache(q, c, tensor_layout=layout, is_causal=True, causal_align="bottom_right", pack_gqa=True, return_lse=True)
            o_ref, l_ref = sc._attn_fused_q(q, ref_k, vi_now, ref_vs, ref_ks, layout, True, sc._sm_log2(sm), True, kv_lens=lens_t,
                                            q_start=sc._q_start_tensor(None, lens_t, B, 1, CAP, DEV), gqa_pack=True)
            o_ref, l_ref = sc._finish(o_ref, l_ref, D, True, True, corr, sm)
            assert torch.equal(o, o_ref), f"{what}: o differs in {int((o != o_ref).sum())} of {o.numel()} elements"
            assert torch.equal(lse, l_ref), f"{what}: lse differs in {int((lse != l_ref).sum())} of {lse.numel()} rows"
            for b, n in enumerate(have):
                assert n > 0 or (bool((o[b] == 0).all()) and bool(torch.isneginf(lse[b]).all())), what
            attended += 1
    assert tuple(have) == final and attended >= 1
    for b, n in enumerate(final):                           # (the last step's reference image is the pre-pass's own, zero tail included)
        assert torch.equal(vi_now[b, :, :(n + 63) // 64], ref_vi[b, :, :(n + 63) // 64]), b


# ---- rows as a caller holds them -------------------------------------------------------------------------------------------------------
# Slices of a larger tensor, no copy made here: the stride arithmetic of both append kernels (k_sl, k_sh, k_sb of real views).  Every element
# around the views holds a NaN bit pattern.  Each append is compared with the same append of a contiguous copy: every byte of the cache.
VIEW_T, VIEW_AT = 70, 30                 # 70 rows behind 30: the rows cross a block end and leave an open block
VIEW_COUNTS = (70, 34, 5, 0)             # ... end exactly on one, stay inside the open block, take nothing
VIEWS = ("narrow_hnd", "narrow_nhd", "packed_qkv", "row_stride_2d", "offset_16_bytes", "offset_8_bytes")


def _nan_like(shape, dt):
    return torch.full(shape, -1, dtype=torch.int16, device=DEV).view(dt)          # 0xFFFF: NaN as fp16 and as bf16


def _views(name, kh, vh, dt):
    """(k view, v view, layout) of rows ``kh`` / ``vh`` [B, HKV, T, D] inside larger NaN-filled tensors."""
    T, D = kh.shape[2], kh.shape[3]
    if name == "narrow_hnd":
        bk, bv = _nan_like((B, HKV, T + 20, D), dt), _nan_like((B, HKV, T + 20, D), dt)
        kv, vv = bk.narrow(2, 7, T), bv.narrow(2, 7, T)
        layout = "HND"
    elif name == "narrow_nhd":
        bk, bv = _nan_like((B, T + 20, HKV, D), dt), _nan_like((B, T + 20, HKV, D), dt)
        kv, vv = bk.narrow(1, 7, T), bv.narrow(1, 7, T)
        layout = "NHD"
    elif name == "packed_qkv":
        qkv = _nan_like((B, T + 9, 3, HKV, D), dt)
        kv, vv = qkv[:, 5:5 + T, 1], qkv[:, 5:5 + T, 2]
        layout = "NHD"
    elif name == "row_stride_2d":
        bk, bv = _nan_like((B, HKV, T + 3, 2 * D), dt), _nan_like((B, HKV, T + 3, 2 * D), dt)
        kv, vv = bk[:, :, 2:2 + T, :D], bv[:, :, 1:1 + T, D:]
        layout = "HND"
    else:
        off = 8 if name == "offset_16_bytes" else 4
        n = B * HKV * T * D
        bk, bv = _nan_like((n + 64,), dt), _nan_like((n + 64,), dt)
        kv, vv = bk[off:off + n].view(B, HKV, T, D), bv[off:off + n].view(B, HKV, T, D)
        layout = "HND"
    kv.copy_(kh if layout == "HND" else kh.transpose(1, 2))
    vv.copy_(vh if layout == "HND" else vh.transpose(1, 2))
    return kv, vv, layout


@pytest.mark.parametrize("name", VIEWS)
@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_appended_views_give_the_bytes_of_a_contiguous_copy(case, name):
    D, dt, _ = case
    k, v, km, v_amax = _content(D, dt, "HND")[:4]
    kh, vh = k[:, :, VIEW_AT:VIEW_AT + VIEW_T], v[:, :, VIEW_AT:VIEW_AT + VIEW_T]
    kv, vv, layout = _views(name, kh, vh, dt)
    assert not kv.is_contiguous() or name.startswith("offset")
    copied = sq._aligned(kv, 8) is not kv                  # which path ran: the wrapper re-packs what is not 16-byte aligned, else the kernels read the view
    print(f"{name}: strides {kv.stride()}, offset {kv.storage_offset()} elements, data_ptr % 16 = {kv.data_ptr() % 16}: "
          f"{'re-packed by the wrapper (a copy)' if copied else 'read in place by the kernels'}")
    assert copied == (name == "offset_8_bytes"), name
    caches = []
    for rows in ((kv, vv, layout), (kh.contiguous(), vh.contiguous(), "HND")):
        c = _poisoned_cache(D, dt)
        c.seed(km, v_amax)
        c.append(k[:, :, :VIEW_AT].contiguous(), v[:, :, :VIEW_AT].contiguous(), _ints([VIEW_AT, VIEW_AT, VIEW_AT, 0]))
        c.append(rows[0], rows[1], _ints(VIEW_COUNTS), rows[2])
        caches.append(c)
    torch.cuda.synchronize()
    a, b_ = caches
    assert a.lens.tolist() == [VIEW_AT + VIEW_COUNTS[0], VIEW_AT + VIEW_COUNTS[1], VIEW_AT + VIEW_COUNTS[2], 0]
    for t in ("k_int8", "k_scale", "v_image", "v_scale", "k_tail", "v_tail", "lens"):
        x, y = _u8(getattr(a, t)), _u8(getattr(b_, t))
        assert torch.equal(x, y), f"{name}: {t} differs in {int((x != y).sum())} bytes from the append of a contiguous copy"
    assert bool((_u8(a.k_int8[0, :, :100]) != POISON).any()) and not bool(torch.isnan(a.k_tail[0, :, :36].float()).any())


# ---- re-seeding ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_a_reseeded_cache_is_a_fresh_one(case):
    """A cache filled to (257, 64, 130, 0), seeded again with other statistics and filled by the "mixed" schedule with other content equals a
    fresh poisoned cache given that seed and schedule wherever the second content defines bytes: the stale tails, scales and tiles of the
    first life reach nothing, the first block included."""
    D, dt, layout = case
    k, v, km, v_amax = _content(*case)[:4]
    seq = 2 if layout == "HND" else 1
    k2 = (0.5 * k.float().flip(seq) + 1.0).to(dt)          # other content: other means, other ranges
    v2 = (1.75 * v.float().roll(11, seq)).to(dt)
    lens = _ints(FINAL)
    km2 = sq.channel_mean_kvlens(k2, lens, layout)
    valid = (torch.arange(CAP, device=DEV)[None, :] < lens[:, None]).view(B, 1, CAP, 1)
    v_amax2 = torch.where(valid, _hnd(v2, layout).abs().float(), 0.0).amax(dim=2)
    assert not torch.equal(km2, km) and not torch.equal(v_amax2, v_amax)
    used = _poisoned_cache(D, dt)
    used.seed(km, v_amax)
    assert tuple(_fill(used, k, v, layout, SCHEDULES["one"])) == FINAL
    used.seed(km2, v_amax2)
    assert used.lens.tolist() == [0] * B
    fresh = _poisoned_cache(D, dt)
    fresh.seed(km2, v_amax2)
    for c in (used, fresh):
        assert tuple(_fill(c, k2, v2, layout, SCHEDULES["mixed"])) == FINAL
    torch.cuda.synchronize()
    assert used.lens.tolist() == fresh.lens.tolist() == list(FINAL)
    assert torch.equal(used.k_mean, fresh.k_mean) and torch.equal(used.v_amax, fresh.v_amax)
    for b, n in enumerate(FINAL):
        nb, r = (n + 63) // 64, n % 64
        for name, sl in (("k_int8", slice(0, n)), ("k_scale", slice(0, nb * 4)), ("v_image", slice(0, nb)), ("k_tail", slice(0, r)), ("v_tail", slice(0, r))):
            x, y = _u8(getattr(used, name)[b, :, sl]), _u8(getattr(fresh, name)[b, :, sl])
            assert torch.equal(x, y), f"sample {b}: {name} differs in {int((x != y).sum())} bytes from the fresh cache"
        if n:
            assert torch.equal(used.v_scale[b].view(torch.int32), fresh.v_scale[b].view(torch.int32)), f"sample {b}: v_scale"
    # ... and both are the pre-pass of the second content
    ref_k, ref_ks = sq.per_thread_int8_k_kvlens(k2, km2, lens, layout)
    ref_vi, _ = sq.per_channel_fp8_kvlens(v2, lens, layout)
    for b, n in enumerate(FINAL):
        nb = (n + 63) // 64
        assert torch.equal(used.k_int8[b, :, :n], _hnd(ref_k, layout)[b, :, :n]) and torch.equal(used.v_image[b, :, :nb], ref_vi[b, :, :nb]), f"sample {b}"
        assert torch.equal(used.k_scale[b, :, :nb * 4].view(torch.int32), ref_ks[b, :, :nb * 4].view(torch.int32)), f"sample {b}"
