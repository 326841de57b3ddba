#!/usr/bin/env python3
"""What packing a GQA group's query heads into one workgroup (pack_gqa=True) does to a decode-shaped call: the packed launch
against the unpacked one, whole calls and the attention kernel alone, interleaved in one process.

Shape: bf16, D 128, Hq 32 / Hkv 8 (groups of four: one workgroup per kv head and sample instead of four), Lk 8192, causal with
causal_align="bottom_right" and kv_lens drawn (seeded) from [Lk / 2, Lk]; Lq 1 (decode) and 16 (speculative verification); B 4, 32 and 128:
B * Hq = 128 workgroups under-fill the 512 resident slots of the chip, 1024 are about two rounds, 4096 many.  Packed, the launches have 32,
256 and 1024 workgroups.

"call" is the whole entry point (pre-pass + attention); "kernel" is the attention launch alone on operands quantised once
(core._attn_fused_q).  Per round every variant is warmed, then timed call by call with device events; the figure of a variant is the median
over the rounds of the round's median, "spread" the range of the round medians relative to it.  The outputs of the two launches are compared
bit for bit before anything is timed.  ``not_slower`` says whether packed <= unpacked * (1 + the larger of the two spreads).

    python tools/gqa_pack_probe.py [--rounds 5] [--reps 10] [--out profiles/gqa_pack_probe.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sageattention_amd as sa  # noqa: E402
from sageattention_amd import core, ops  # noqa: E402

HQ, HKV, LK, D = 32, 8, 8192, 128
BATCHES, LQS = (4, 32, 128), (1, 16)


def variants(q, k, v, lens):
    """{"unpacked" / "packed": callable} for the whole call and for the kernel alone, on one (B, Lq)."""
    B, Lq = q.shape[0], q.shape[2]
    sm = core._sm_log2(D ** -0.5)
    _, _, k8, ks, vimg, vs, _ = core._prepass_kv(q, k, v, "HND", "per_thread", 64, True, False, False, False, kv_lens=lens)
    qs = core._q_start_tensor(None, lens, B, Lq, LK, q.device)
    calls, kernels = {}, {}
    for name, on in (("unpacked", False), ("packed", True)):
        calls[name] = lambda on=on: sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=True, pv_accum_dtype="fp32+fp32", kv_lens=lens,
                                                                    causal_align="bottom_right", pack_gqa=on)
        kernels[name] = lambda on=on: core._attn_fused_q(q, k8, vimg, vs, ks, "HND", True, sm, False, kv_lens=lens, q_start=qs, gqa_pack=on)[0]
    return calls, kernels


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
    out["packed_over_unpacked"] = round(out["packed"]["us"] / out["unpacked"]["us"], 4)
    out["not_slower"] = out["packed"]["us"] <= out["unpacked"]["us"] * (1.0 + max(out["packed"]["spread"], out["unpacked"]["spread"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gqa_pack_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gqa_pack_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(14)
    bmax = max(BATCHES)
    k_all, v_all = (torch.randn(bmax, HKV, LK, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(2))
    q_all = torch.randn(bmax, HQ, max(LQS), D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    lens_all = torch.randint(LK // 2, LK + 1, (bmax,), generator=torch.Generator().manual_seed(14)).to(torch.int32)
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D 128, Hq 32 / Hkv 8, Lk 8192, "
                   "causal_align='bottom_right' with kv_lens drawn from [Lk / 2, Lk]; call = whole entry point, kernel = attention launch alone; "
                   "spread = range of the round medians / the figure; not_slower = packed <= unpacked * (1 + the larger spread)",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "shapes": []}
    for B in BATCHES:
        for Lq in LQS:
            q, k, v = q_all[:B, :, :Lq].contiguous(), k_all[:B], v_all[:B]
            lens = lens_all[:B].to(dev)
            calls, kernels = variants(q, k, v, lens)
            probe, grids = ctypes.c_int32(-1), {}
            outs = {}
            for n, fn in calls.items():
                with ops.launch_hooks(grid_probe=probe):
                    outs[n] = fn()
                grids[n] = probe.value
            assert torch.equal(outs["packed"], outs["unpacked"]), "the packed launch must give the unpacked launch's bits"
            assert torch.equal(kernels["packed"](), kernels["unpacked"]())
            assert grids == {"unpacked": B * HQ, "packed": B * HKV * ((HQ // HKV + 3) // 4)}, grids
            r = {"B": B, "Lq": Lq, "workgroups": grids, "lens_min_max": [int(lens.min()), int(lens.max())],
                 "kernel": summary(time_interleaved(kernels, a.rounds, a.reps)), "call": summary(time_interleaved(calls, a.rounds, a.reps))}
            res["shapes"].append(r)
            for what in ("kernel", "call"):
                s = r[what]
                print(f"B {B:3d} Lq {Lq:2d} {what:6s} unpacked {s['unpacked']['us']:8.1f} us (spread {s['unpacked']['spread']:.3f}, {grids['unpacked']} wg)  "
                      f"packed {s['packed']['us']:8.1f} us (spread {s['packed']['spread']:.3f}, {grids['packed']} wg)  "
                      f"packed / unpacked x{s['packed_over_unpacked']:.4f}  not slower: {s['not_slower']}", flush=True)
    res["not_slower_everywhere"] = all(r[w]["not_slower"] for r in res["shapes"] for w in ("kernel", "call"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
