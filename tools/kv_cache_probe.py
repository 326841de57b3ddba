#!/usr/bin/env python3
"""What the appendable quantised KV cache (sageattention_amd.kv_cache) does to one decode step: append one row and attend to
the cache, against today's one-shot call that runs the whole K / V pre-pass over the whole context, interleaved in one process.

Shape (that of tools/gqa_pack_probe.py): bf16, D 128, Hq 32 / Hkv 8, Lk 8192 (the one-shot call's padded length and the cache's capacity),
Lq 1, causal with causal_align="bottom_right", pack_gqa=True; B 4, 32 and 128; the lengths before the step drawn (seeded) from
[Lk / 2, Lk - 1], the step adds row ``len_b`` of every sample.

"oneshot"  sageattn_qk_int8_pv_fp8_cuda(q, k, v, kv_lens=len + 1, ...) on tensors that hold the new row (code this probe's subject does not touch)
"cached"   cache.append(one row) + sageattn_kvcache(q, cache, ...)                             -- the whole step
"append"   cache.append(one row) alone: the two kernels of sage_kvcache_append
"kernel"   the attention launch alone on the cache's operands (core._attn_fused_q)
Before every timed "cached" / "append" call the cache's lengths are put back to the drawn ones, outside the timed interval, so every call of
a variant does the same work.  The cache is seeded with the statistics of its final content, so that before anything is timed the cached
step's output can be compared with the one-shot call's bit for bit.

Per round every variant is warmed, then timed call by call with device events; the figure of a variant is the median over the rounds of the
round's median, "spread" the range of the round medians relative to it.

    python tools/kv_cache_probe.py [--rounds 5] [--reps 10] [--out profiles/kv_cache_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sageattention_amd as sa  # noqa: E402
from sageattention_amd import core, quant  # noqa: E402
from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache  # noqa: E402

HQ, HKV, LK, D = 32, 8, 8192, 128
BATCHES, LQ = (4, 32, 128), 1
KW = dict(is_causal=True, causal_align="bottom_right", pack_gqa=True)


def variants(q, k, v, lens):
    """{name: (untimed setup, timed call)} on one batch; ``k`` / ``v`` hold row ``lens[b]``, the row the step adds."""
    B = q.shape[0]
    lens1 = lens + 1
    idx = lens.long().view(B, 1, 1, 1).expand(B, HKV, 1, D)
    k_row, v_row = k.gather(2, idx).contiguous(), v.gather(2, idx).contiguous()
    valid = (torch.arange(LK, device=q.device)[None, :] < lens1[:, None]).view(B, 1, LK, 1)
    cache = QuantizedKVCache.allocate(B, HKV, LK, D, q.dtype, q.device)
    cache.seed(quant.channel_mean_kvlens(k, lens1), torch.where(valid, v.abs().float(), 0.0).amax(dim=2))
    cache.append(k, v, lens)
    sm = core._sm_log2(D ** -0.5)
    qs = core._q_start_tensor(None, lens1, B, LQ, LK, q.device)
    reset = lambda: cache.lens.copy_(lens)
    nothing = lambda: None

    def cached():
        cache.append(k_row, v_row)
        return sageattn_kvcache(q, cache, **KW)

    fns = {
        "oneshot": (nothing, lambda: sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, pv_accum_dtype="fp32+fp32", kv_lens=lens1, **KW)),
        "cached": (reset, cached),
        "append": (reset, lambda: cache.append(k_row, v_row)),
        "kernel": (nothing, lambda: core._attn_fused_q(q, cache.k_int8, cache.v_image, cache.v_scale, cache.k_scale, "HND", True, sm, False,
                                                       kv_lens=lens1, q_start=qs, gqa_pack=True)[0]),
    }
    reset()
    o_cached, o_shot = fns["cached"][1](), fns["oneshot"][1]()
    assert torch.equal(o_cached, o_shot), "seeded with the final statistics, the cached step must give the one-shot call's bits"
    assert torch.equal(cache.lens, lens1)
    return fns


def time_interleaved(fns, rounds, reps):
    """us per call: {variant: [median of round 0, round 1, ...]}"""
    per_round = {n: [] for n in fns}
    for _ in range(rounds):
        for n, (setup, fn) in fns.items():
            for _ in range(3):
                setup()
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                setup()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record(); b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            per_round[n].append(statistics.median(ts))
    return per_round


def summary(per_round):
    out = {}
    for n, xs in per_round.items():
        med = statistics.median(xs)
        out[n] = {"us": round(med, 1), "spread": round((max(xs) - min(xs)) / med, 4), "us_rounds": [round(x, 1) for x in xs]}
    out["cached_over_oneshot"] = round(out["cached"]["us"] / out["oneshot"]["us"], 4)
    out["cached_over_kernel"] = round(out["cached"]["us"] / out["kernel"]["us"], 4)
    out["cached_below_oneshot"] = out["cached"]["us"] < out["oneshot"]["us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_cache_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kv_cache_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(16)
    bmax = max(BATCHES)
    k_all, v_all = (torch.randn(bmax, HKV, LK, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(2))
    q_all = torch.randn(bmax, HQ, LQ, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    lens_all = torch.randint(LK // 2, LK, (bmax,), generator=torch.Generator().manual_seed(16)).to(torch.int32)
    res = {"what": "us per decode step, median over interleaved rounds of the round's median (device events); bf16, D 128, Hq 32 / Hkv 8, Lk 8192 "
                   "(padded length and cache capacity), Lq 1, causal_align='bottom_right', pack_gqa=True, lengths drawn from [Lk / 2, Lk - 1] plus the "
                   "step's row; oneshot = sageattn_qk_int8_pv_fp8_cuda(kv_lens=) whole call, cached = append(1 row) + sageattn_kvcache whole call, "
                   "append = the two kernels of sage_kvcache_append through cache.append, kernel = the attention launch alone on the cache; "
                   "spread = range of the round medians / the figure",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "shapes": []}
    for B in BATCHES:
        q, k, v = q_all[:B], k_all[:B], v_all[:B]
        lens = lens_all[:B].to(dev)
        r = {"B": B, "Lq": LQ, "lens_min_max": [int(lens.min()), int(lens.max())]}
        r.update(summary(time_interleaved(variants(q, k, v, lens), a.rounds, a.reps)))
        res["shapes"].append(r)
        print(f"B {B:3d} oneshot {r['oneshot']['us']:8.1f} us (spread {r['oneshot']['spread']:.3f})  cached {r['cached']['us']:8.1f} us "
              f"(spread {r['cached']['spread']:.3f})  append {r['append']['us']:7.1f} us  kernel {r['kernel']['us']:8.1f} us  "
              f"cached / oneshot x{r['cached_over_oneshot']:.4f}  cached / kernel x{r['cached_over_kernel']:.4f}", flush=True)
    res["cached_below_oneshot_everywhere"] = all(r["cached_below_oneshot"] for r in res["shapes"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
