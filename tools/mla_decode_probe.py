#!/usr/bin/env python3
"""First numbers of the absorbed MLA decode route (sageattention_amd.mla_decode): the attention launch alone, the pre-pass alone, the
whole call, and the route a caller has today, interleaved in one run on the same inputs:

  sdpa    torch.nn.functional.scaled_dot_product_attention on the bf16 operands: the one latent "kv head" serves all heads, so the heads are
          folded into the query rows (q [B, 1, Lq * Hq, 576] -- the cheapest way to broadcast K over the heads), V is the latent's first 512
          channels zero-padded to 576 (once, outside the timed call), and the mask is a lower-right boolean bias built outside as well.

  bf16, Hq 128, Lq 1 and 2, B 32 / 128 / 256, contexts 4096 and 8192, lengths uniform in [Lk / 2, Lk].

Per (shape, variant): us = the median over the rounds of the round's median (device events around one call), spread = (max - min) / median of
the round medians.  For the attention launch also the achieved bytes per second, sum(kv_lens) * 1088 / time, against 8 TB/s, and TFLOP/s on
2 * 1088 per (row, visible key).  Every variant is warmed up at every shape before the first timed round, and the new route's output is
compared with sdpa's at every shape.  No figure is a gate.

    python tools/mla_decode_probe.py [--rounds 5] [--reps 10] [--out profiles/mla_decode_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from sageattention_amd.mla_decode import mla_quantize_latent, sageattn_mla_decode  # noqa: E402

HQ, DQK, DV = 128, 576, 512


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mla_decode_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(9)
    variants, agree = {}, {}
    for Lk in (4096, 8192):
        for B in (32, 128, 256):
            kv = torch.randn(B, Lk, DQK, generator=g).to(torch.bfloat16).to(dev)
            lens_h = torch.randint(Lk // 2, Lk + 1, (B,), generator=g)
            lens = lens_h.to(torch.int32).to(dev)
            lat = mla_quantize_latent(kv, lens)
            k1, v1 = kv[:, None], F.pad(kv[..., :DV], (0, DQK - DV))[:, None]
            for Lq in (1, 2):
                q = torch.randn(B, Lq, HQ, DQK, generator=g).to(torch.bfloat16).to(dev)
                vis = (lens_h[:, None] - Lq + 1 + torch.arange(Lq)[None, :]).clamp(min=0)                  # [B, Lq] visible keys
                bias = (torch.arange(Lk)[None, None, :] < vis[:, :, None]).repeat_interleave(HQ, dim=1)[:, None].to(dev)
                q1 = q.reshape(B, 1, Lq * HQ, DQK)
                pairs = float(vis.sum()) * HQ
                variants[f"B{B}_Lk{Lk}_Lq{Lq}"] = dict(
                    flops=2.0 * (DQK + DV) * pairs, bytes=float(lens_h.sum()) * (DQK + DV),
                    fns=dict(attn=lambda q=q, lat=lat: sageattn_mla_decode(q, lat),
                             prepass=lambda kv=kv, lens=lens: mla_quantize_latent(kv, lens),
                             call=lambda q=q, kv=kv, lens=lens: sageattn_mla_decode(q, kv, lens),
                             sdpa=lambda q1=q1, k1=k1, v1=v1, bias=bias, B=B, Lq=Lq: F.scaled_dot_product_attention(
                                 q1, k1, v1, attn_mask=bias).reshape(B, Lq, HQ, DQK)[..., :DV]))
    for t, var in variants.items():             # warm-up: every variant at every shape; and what the new route computes against sdpa
        for fn in var["fns"].values():
            for _ in range(2):
                fn()
        o, r = var["fns"]["attn"]().float(), var["fns"]["sdpa"]().float()
        agree[t] = dict(max_abs_diff=round((o - r).abs().max().item(), 5), max_abs_ref=round(r.abs().max().item(), 5))
    torch.cuda.synchronize()
    rounds = {(t, n): [] for t, var in variants.items() for n in var["fns"]}
    for _ in range(a.rounds):                   # interleaved: one round visits every (shape, variant)
        for t, var in variants.items():
            for n, fn in var["fns"].items():
                rounds[(t, n)].append(timed(fn, a.reps))
    out = dict(device=torch.cuda.get_device_name(0), shape=dict(Hq=HQ, Dqk=DQK, Dv=DV, dtype="bf16"), rounds=a.rounds, reps=a.reps,
               output_against_sdpa=agree, results={})
    for (t, n), meds in rounds.items():
        us = statistics.median(meds)
        r = dict(us=round(us, 1), spread=round((max(meds) - min(meds)) / us, 4), round_medians_us=[round(m, 1) for m in meds])
        if n in ("attn", "sdpa"):
            r["tflops"] = round(variants[t]["flops"] / us * 1e-6, 1)
        if n == "attn":
            r["tbytes_per_s"] = round(variants[t]["bytes"] / us * 1e-6, 3)
            r["of_8_tb_per_s"] = round(variants[t]["bytes"] / us * 1e-6 / 8.0, 3)
        out["results"].setdefault(t, {})[n] = r
        print(f"{t:18s} {n:8s} {us:9.1f} us  spread {r['spread']:.3f}  " + " ".join(f"{k} {v}" for k, v in r.items() if k.startswith("t")))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
