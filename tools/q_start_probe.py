#!/usr/bin/env python3
"""What per-sample query offsets (q_start / causal_align="bottom_right") cost at a chunked-prefill shape: whole calls and the attention
kernel alone, four ways, interleaved.

  plain_tl       sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=True)          (top-left: row i sees keys <= i -- the first Lq keys only)
  kv_tl          ... kv_lens = lens                                              (the same top-left mask through the kv_lens route)
  br_aligned     ... kv_lens = lens, causal_align="bottom_right"                 (lens multiples of 64: offsets lens - Lq are multiples of 64,
                                                                                  the diagonal tiles keep the pipelined last-tile bodies)
  br_unaligned   ... kv_lens = lens - 23, causal_align="bottom_right"            (offsets that are no multiple of 64: the diagonal of every
                                                                                  query block runs as three general tiles)

Shape: B2 H32 D128 bf16, Lk 8192, Lq 512 new rows, lens drawn (seeded) from [Lk / 2, Lk] in steps of 64.  The bottom-right variants attend to
len_b - Lq + i + 1 keys per row -- about Lk * 3 / 4 on average -- where the top-left ones attend to i + 1 <= Lq: they are different amounts of
work, so the bottom-right figures are also given per attended (row, key) pair.  br_unaligned against br_aligned is the same work but for 23 keys
per row: its ratio is what the three-tile diagonal costs.  "call" is the whole entry point (pre-pass + attention); "kernel" is the attention
launch alone on operands quantised once (core._attn_fused_q).  Per round every variant is warmed, then timed call by call with device
events; the figure of a variant is the median over the rounds of the round's median, "spread" the range of the round medians relative to it.

    python tools/q_start_probe.py [--rounds 5] [--reps 10] [--out profiles/q_start_probe.json]
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

SHAPE = dict(name="chunked_prefill_b2_h32_lq512_lk8192_d128", B=2, H=32, Lq=512, Lk=8192)
UNALIGN = 23


def variants(c, dev):
    g = torch.Generator(device="cpu").manual_seed(11)
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    q = torch.randn(B, H, Lq, 128, generator=g).to(torch.bfloat16).to(dev)
    k, v = (torch.randn(B, H, Lk, 128, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    drawn = 64 * torch.randint(Lk // 128, Lk // 64 + 1, (B,), generator=g)
    lens = drawn.to(torch.int32).to(dev)
    # name -> (kv_lens, bottom-right?)
    spec = {"plain_tl": (None, False), "kv_tl": (lens, False), "br_aligned": (lens, True), "br_unaligned": (lens - UNALIGN, True)}
    sm = core._sm_log2(128 ** -0.5)
    calls, kernels = {}, {}
    for name, (kl, br) in spec.items():
        kw = dict(causal_align="bottom_right") if br else {}
        calls[name] = lambda kl=kl, kw=kw: sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=True, pv_accum_dtype="fp32+fp32", kv_lens=kl, **kw)
        fused = core._fused_prepass_wanted(k, "HND", None)
        _, _, k8, ks, vimg, vs, _ = core._prepass_kv(q, k, v, "HND", "per_thread", 64, True, False, False, fused, kv_lens=kl)
        qs = core._q_start_tensor(None, kl, B, Lq, Lk, dev) if br else None
        kernels[name] = lambda k8=k8, ks=ks, vimg=vimg, vs=vs, kl=kl, qs=qs: core._attn_fused_q(q, k8, vimg, vs, ks, "HND", True, sm, False, kv_lens=kl, q_start=qs)
    n = [int(x) for x in drawn]
    pairs = {"plain_tl": B * H * Lq * (Lq + 1) // 2, "kv_tl": B * H * Lq * (Lq + 1) // 2,
             "br_aligned": H * sum(Lq * (x - Lq) + Lq * (Lq + 1) // 2 for x in n),
             "br_unaligned": H * sum(Lq * (x - UNALIGN - Lq) + Lq * (Lq + 1) // 2 for x in n)}
    return calls, kernels, n, pairs, (q, k, v)


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


def summary(per_round, pairs):
    out = {}
    for n, xs in per_round.items():
        med = statistics.median(xs)
        out[n] = {"us": round(med, 1), "spread": round((max(xs) - min(xs)) / med, 4), "us_rounds": [round(x, 1) for x in xs],
                  "ps_per_row_key_pair": round(med * 1e6 / pairs[n], 4)}
    out["kv_tl_over_plain_tl"] = round(out["kv_tl"]["us"] / out["plain_tl"]["us"], 4)
    out["br_unaligned_over_br_aligned"] = round(out["br_unaligned"]["us"] / out["br_aligned"]["us"], 4)
    out["br_aligned_over_plain_tl"] = round(out["br_aligned"]["us"] / out["plain_tl"]["us"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q_start_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "q_start_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    c = SHAPE
    calls, kernels, drawn, pairs, qkv = variants(c, dev)
    assert torch.equal(calls["plain_tl"](), sa.sageattn_qk_int8_pv_fp8_cuda(*qkv, is_causal=True, pv_accum_dtype="fp32+fp32", q_start=0)), \
        "q_start = 0 must be the plain causal call, bit for bit"
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D = 128, causal; call = whole entry "
                   "point, kernel = attention launch alone; spread = range of the round medians / the figure; ps_per_row_key_pair = the figure "
                   "over the (row, key) pairs the variant attends to (the top-left variants attend to the first Lq keys only)",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps,
           "shape": {kk: c[kk] for kk in ("B", "H", "Lq", "Lk")}, "lens": drawn, "unaligned_lens": [x - UNALIGN for x in drawn],
           "attended_row_key_pairs": pairs,
           "call": summary(time_interleaved(calls, a.rounds, a.reps), pairs), "kernel": summary(time_interleaved(kernels, a.rounds, a.reps), pairs)}
    print(c["name"], "lens", drawn, flush=True)
    for what in ("call", "kernel"):
        r = res[what]
        print(f"  {what:6s} " + "  ".join(f"{n} {r[n]['us']:8.1f} us (spread {r[n]['spread']:.3f})" for n in calls), flush=True)
        print(f"         kv_tl / plain_tl x{r['kv_tl_over_plain_tl']:.4f}   br_unaligned / br_aligned x{r['br_unaligned_over_br_aligned']:.4f}   "
              f"ps per pair: aligned {r['br_aligned']['ps_per_row_key_pair']:.4f}, unaligned {r['br_unaligned']['ps_per_row_key_pair']:.4f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
