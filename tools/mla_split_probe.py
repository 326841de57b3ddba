#!/usr/bin/env python3
"""What the exact split of the key range buys the absorbed MLA decode call (sageattn_mla_decode(num_splits=)), by the method of
tools/mla_decode_probe.py: the unsplit attention launch -- the kernel of DESIGN 3.29, unchanged -- next to the whole split call (pass 1, pass 2
and the merge, with its workspace allocation) at S = 2, 4, 8, 16, 32, on one quantised latent, interleaved in one run.

  bf16, Hq 128, Lq 1 and 2, B 1 / 8 / 32 / 128, contexts 4096 / 8192 / 32768, lengths uniform in [Lk / 2, Lk].

Per (shape, variant): us = the median over the rounds of the round's median (device events around one call), spread = (max - min) / median of
the round medians.  Every variant is warmed up at every shape before the first timed round, and the split call's output is compared with the
unsplit call's at every shape.  The three launches are not timed apart: the C entry issues them back to back.  No figure is a gate; the
constants of the ``"auto"`` plan (sageattention_amd/mla_decode.py) are read off this table.

    python tools/mla_split_probe.py [--rounds 5] [--reps 10] [--out profiles/mla_split_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sageattention_amd.mla_decode import mla_quantize_latent, sageattn_mla_decode  # noqa: E402
from mla_decode_probe import DQK, HQ, timed  # noqa: E402

SPLITS = (2, 4, 8, 16, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mla_split_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(9)
    variants, agree = {}, {}
    for Lk in (4096, 8192, 32768):
        for B in (1, 8, 32, 128):
            kv = torch.randn(B, Lk, DQK, generator=g, device=dev).to(torch.bfloat16)
            lens = torch.randint(Lk // 2, Lk + 1, (B,), generator=g, device=dev).to(torch.int32)
            lat = mla_quantize_latent(kv, lens)
            del kv
            for Lq in (1, 2):
                q = torch.randn(B, Lq, HQ, DQK, generator=g, device=dev).to(torch.bfloat16)
                fns = {"unsplit": lambda q=q, lat=lat: sageattn_mla_decode(q, lat)}
                for S in SPLITS:
                    fns[f"S{S}"] = lambda q=q, lat=lat, S=S: sageattn_mla_decode(q, lat, num_splits=S)
                variants[f"B{B}_Lk{Lk}_Lq{Lq}"] = fns
    for t, fns in variants.items():             # warm-up: every variant at every shape; and the split's output against the unsplit call's
        for fn in fns.values():
            for _ in range(2):
                fn()
        r = fns["unsplit"]().float()
        agree[t] = dict(max_abs_diff=max(round((fns[f"S{S}"]().float() - r).abs().max().item(), 5) for S in SPLITS),
                        max_abs_ref=round(r.abs().max().item(), 5))
    torch.cuda.synchronize()
    rounds = {(t, n): [] for t, fns in variants.items() for n in fns}
    for _ in range(a.rounds):                   # interleaved: one round visits every (shape, variant)
        for t, fns in variants.items():
            for n, fn in fns.items():
                rounds[(t, n)].append(timed(fn, a.reps))
    out = dict(device=torch.cuda.get_device_name(0), shape=dict(Hq=HQ, Dqk=DQK, Dv=512, dtype="bf16"), rounds=a.rounds, reps=a.reps,
               output_against_unsplit=agree, results={})
    for (t, n), meds in rounds.items():
        us = statistics.median(meds)
        out["results"].setdefault(t, {})[n] = dict(us=round(us, 1), spread=round((max(meds) - min(meds)) / us, 4),
                                                   round_medians_us=[round(m, 1) for m in meds])
    for t, res in out["results"].items():
        base = res["unsplit"]["us"]
        for n, r in res.items():
            r["of_unsplit"] = round(r["us"] / base, 3)
        print(f"{t:18s} unsplit {base:8.1f} us (spread {res['unsplit']['spread']:.3f})  " +
              "  ".join(f"{n} x{res[n]['of_unsplit']:.2f} ({res[n]['spread']:.2f})" for n in res if n != "unsplit"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
