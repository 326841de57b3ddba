#!/usr/bin/env python3
"""What per-sample key lengths (kv_lens) cost and buy: whole calls and the attention kernel alone, three ways per shape, interleaved.

  plain      sageattn_qk_int8_pv_fp8_cuda(q, k, v)                        (the padded call: every key attended to)
  kv_full    ... kv_lens = [Lk] * B                                        (the same work through the kv_lens route: what the flag costs)
  kv_drawn   ... kv_lens drawn uniformly from [Lk / 4, Lk] (seeded)        (what the skipped keys buy against the padded call)

Shapes (bf16, D = 128, non-causal): B2 H32 N8192, and a Wan-like cross-attention B2 H40 Lq 32760 Lk 512.  "call" is the whole entry point
(pre-pass + attention); "kernel" is the attention launch alone on operands quantised once (core._attn_fused_q).  Per round every variant
is warmed, then timed call by call with device events; the figure of a variant is the median over the rounds of the round's median, and
"spread" is the range of the round medians relative to that figure.

    python tools/kv_lens_probe.py [--rounds 5] [--reps 10] [--out profiles/kv_lens_probe.json]
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
from sageattention_amd import core  # noqa: E402

SHAPES = [dict(name="b2_h32_n8192_d128", B=2, H=32, Lq=8192, Lk=8192), dict(name="wan_cross_b2_h40_lq32760_lk512_d128", B=2, H=40, Lq=32760, Lk=512)]


def variants(c, dev):
    g = torch.Generator(device="cpu").manual_seed(11)
    q = torch.randn(c["B"], c["H"], c["Lq"], 128, generator=g).to(torch.bfloat16).to(dev)
    k, v = (torch.randn(c["B"], c["H"], c["Lk"], 128, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    drawn = torch.randint(c["Lk"] // 4, c["Lk"] + 1, (c["B"],), generator=g)
    lens = {"plain": None, "kv_full": torch.full((c["B"],), c["Lk"], dtype=torch.int32, device=dev), "kv_drawn": drawn.to(torch.int32).to(dev)}
    sm = core._sm_log2(128 ** -0.5)
    calls, kernels = {}, {}
    for name, kl in lens.items():
        calls[name] = lambda kl=kl: sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, pv_accum_dtype="fp32+fp32", kv_lens=kl)
        fused = core._fused_prepass_wanted(k, "HND", None)
        _, _, k8, ks, vimg, vs, _ = core._prepass_kv(q, k, v, "HND", "per_thread", 64, True, False, False, fused, kv_lens=kl)
        kernels[name] = lambda k8=k8, ks=ks, vimg=vimg, vs=vs, kl=kl: core._attn_fused_q(q, k8, vimg, vs, ks, "HND", False, sm, False, kv_lens=kl)
    return calls, kernels, [int(x) for x in drawn]


def time_interleaved(fns, rounds, reps):
    """us per call: {variant: [median of round 0, round 1, ...]}"""
    per_round = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
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
    out["kv_full_over_plain"] = round(out["kv_full"]["us"] / out["plain"]["us"], 4)
    out["kv_drawn_over_plain"] = round(out["kv_drawn"]["us"] / out["plain"]["us"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_lens_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kv_lens_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D = 128, non-causal; "
                   "call = whole entry point, kernel = attention launch alone; spread = range of the round medians / the figure",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "shapes": {}}
    for c in SHAPES:
        calls, kernels, drawn = variants(c, dev)
        full, plain = calls["kv_full"](), calls["plain"]()
        assert torch.equal(full, plain), "all lengths full must be the plain call, bit for bit"
        row = {"shape": {kk: c[kk] for kk in ("B", "H", "Lq", "Lk")}, "kv_drawn_lens": drawn,
               "call": summary(time_interleaved(calls, a.rounds, a.reps)), "kernel": summary(time_interleaved(kernels, a.rounds, a.reps))}
        res["shapes"][c["name"]] = row
        print(c["name"], "drawn", drawn, flush=True)
        for what in ("call", "kernel"):
            r = row[what]
            print(f"  {what:6s} plain {r['plain']['us']:9.1f} us (spread {r['plain']['spread']:.3f})  kv_full {r['kv_full']['us']:9.1f} "
                  f"(x{r['kv_full_over_plain']:.4f})  kv_drawn {r['kv_drawn']['us']:9.1f} (x{r['kv_drawn_over_plain']:.4f})", flush=True)
        del calls, kernels
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
