#!/usr/bin/env python3
"""What the appendable quantised latent buys one decode step of the absorbed MLA call (sageattention_amd.mla_cache), by the method
of tools/mla_decode_probe.py: one interleaved run, device events around one call, five rounds of ten.

  bf16, Hq 128, Lq 1, B 32 / 128, contexts 4096 / 8192, lengths uniform in [Lk / 2, Lk - 256] (room for every appended row of the run).

Variants per shape:
  prepass_route   sageattn_mla_decode(q, kv, kv_lens): the three-launch pre-pass over the whole latent, then the attention launch -- the only
                  route without the cache;
  cache_step      cache.append(one row per sample) + sageattn_mla_decode(q, cache.latent()): one decode step on the cache;
  append          the append's two launches alone;
  attention       sageattn_mla_decode(q, cache.latent()) alone (the attention launch of both routes, on the cache's tensors).
The cache grows by one row per timed append, so the open tile of a sample is re-quantised at every fill from 1 to 64 over the run.

Per (shape, variant): us = the median over the rounds of the round's median, spread = (max - min) / median of the round medians.  Every variant
is warmed up at every shape before the first timed round, and the cache step's output is compared with the pre-pass route's on the same rows
(the statistics differ -- frozen prompt statistics with head-room 2 against the final content's -- so the two are not bit-equal).  No figure is
a gate.

    python tools/mla_cache_probe.py [--rounds 5] [--reps 10] [--out profiles/mla_cache_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sageattention_amd.mla_cache import MlaLatentCache  # noqa: E402
from sageattention_amd.mla_decode import sageattn_mla_decode  # noqa: E402
from mla_decode_probe import DQK, HQ, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mla_cache_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    assert 2 * (a.rounds * a.reps + 3) <= 256, "the lengths leave room for 256 appended rows"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(9)
    variants, agree = {}, {}
    for Lk in (4096, 8192):
        for B in (32, 128):
            kv = torch.randn(B, Lk, DQK, generator=g, device=dev).to(torch.bfloat16)
            lens = torch.randint(Lk // 2, Lk - 255, (B,), generator=g, device=dev).to(torch.int32)
            q = torch.randn(B, 1, HQ, DQK, generator=g, device=dev).to(torch.bfloat16)
            row = torch.randn(B, 1, DQK, generator=g, device=dev).to(torch.bfloat16)
            cache = MlaLatentCache.from_prefill(kv, lens, capacity=Lk)

            def step(cache=cache, q=q, row=row):
                cache.append(row)
                return sageattn_mla_decode(q, cache.latent())

            variants[f"B{B}_Lk{Lk}"] = {"prepass_route": lambda q=q, kv=kv, lens=lens: sageattn_mla_decode(q, kv, lens),
                                        "cache_step": step,
                                        "append": lambda cache=cache, row=row: cache.append(row),
                                        "attention": lambda cache=cache, q=q: sageattn_mla_decode(q, cache.latent())}
            # the same rows through both routes: the prompt as it stands
            r = sageattn_mla_decode(q, kv, lens).float()
            agree[f"B{B}_Lk{Lk}"] = dict(max_abs_diff=round((sageattn_mla_decode(q, cache.latent()).float() - r).abs().max().item(), 5),
                                         max_abs_ref=round(r.abs().max().item(), 5))
    for fns in variants.values():               # warm-up: every variant at every shape
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    rounds = {(t, n): [] for t, fns in variants.items() for n in fns}
    for _ in range(a.rounds):                   # interleaved: one round visits every (shape, variant)
        for t, fns in variants.items():
            for n, fn in fns.items():
                rounds[(t, n)].append(timed(fn, a.reps))
    out = dict(device=torch.cuda.get_device_name(0), shape=dict(Hq=HQ, Lq=1, Dqk=DQK, Dv=512, dtype="bf16"), rounds=a.rounds, reps=a.reps,
               cache_against_prepass_route=agree, results={})
    for (t, n), meds in rounds.items():
        us = statistics.median(meds)
        out["results"].setdefault(t, {})[n] = dict(us=round(us, 1), spread=round((max(meds) - min(meds)) / us, 4),
                                                   round_medians_us=[round(m, 1) for m in meds])
    for t, res in out["results"].items():
        base = res["prepass_route"]["us"]
        for r in res.values():
            r["of_prepass_route"] = round(r["us"] / base, 3)
        print(f"{t:12s} " + "  ".join(f"{n} {r['us']:8.1f} us x{r['of_prepass_route']:.2f} ({r['spread']:.2f})" for n, r in res.items()))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
