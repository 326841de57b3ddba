#!/usr/bin/env python3
"""What the exact split of the kv_lens family (num_splits=) does to decode-shaped calls with few sequences: the packed launch
without a split against S = 2 ... 32 key-range chunks and the auto plan, whole calls and the attention launches alone, interleaved in one process.

Shape: bf16, D 128, Hq 32 / Hkv 8, causal with causal_align="bottom_right" and kv_lens drawn (seeded) from [Lk / 2, Lk], with pack_gqa=True
and without; Lq 1 (decode) and 16 (speculative verification); B 1 ... 32; Lk 8192, 32768 and 65536.  Unsplit, the launches have B * 8
workgroups packed and B * 32 unpacked, on 256 compute units.  ``auto_ok`` says that the auto plan chose no split or one that is faster
(kernel and call).

"call" is the whole entry point (pre-pass + attention); "kernel" is the attention entry alone on operands quantised once (core._attn_fused_q:
one launch unsplit, pass 1 + pass 2 + merge with a split -- the three launches summed).  Per round every variant is warmed, then timed call by
call with device events; the figure of a variant is the median over the rounds of the round's median, "spread" the range of the round medians
relative to it.  Every split output is compared with the unsplit one (2 output ulps + 1e-5 max|o|) before anything is timed.  ``faster`` says
whether variant < unsplit * (1 - the larger of the two spreads): the yardstick is the unsplit packed call in the same process, no threshold.

(tools/kv_split_probe.py is an older probe of the FP16-PV pre-pass's halves; this one has a name of its own.)

    python tools/num_splits_probe.py [--rounds 5] [--reps 8] [--out profiles/num_splits_probe.json] [--lk 8192,32768,65536] [--batches 1,2,4,8,16,32]
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

HQ, HKV, D = 32, 8, 128
LQS = (1, 16)
SPLITS = (2, 4, 8, 16, 32)


def variants(q, k, v, lens, Lk, packed):
    """{"unsplit" / "s2" ... / "auto": callable} for the whole call and for the attention entry alone, on one (B, Lq, Lk), with or without
    pack_gqa; the auto plan's S."""
    B, Lq = q.shape[0], q.shape[2]
    sm = core._sm_log2(D ** -0.5)
    _, _, k8, ks, vimg, vs, _ = core._prepass_kv(q, k, v, "HND", "per_thread", 64, True, False, False, False, kv_lens=lens)
    qs = core._q_start_tensor(None, lens, B, Lq, Lk, q.device)
    auto = core._num_splits_plan(B, HQ, HKV, Lq, Lk, packed)
    calls, kernels = {}, {}
    for name, s in [("unsplit", None)] + [(f"s{s}", s) for s in SPLITS] + [("auto", "auto")]:
        n = auto if s == "auto" else (s or 0)
        calls[name] = lambda s=s: sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=True, pv_accum_dtype="fp32+fp32", kv_lens=lens,
                                                                  causal_align="bottom_right", pack_gqa=packed or None, num_splits=s)
        kernels[name] = lambda n=n: core._attn_fused_q(q, k8, vimg, vs, ks, "HND", True, sm, False, kv_lens=lens, q_start=qs, gqa_pack=packed,
                                                       num_splits=n)[0]
    return calls, kernels, auto


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
    base = out["unsplit"]
    for n in per_round:
        if n != "unsplit":
            out[n]["over_unsplit"] = round(out[n]["us"] / base["us"], 4)
            out[n]["faster"] = out[n]["us"] < base["us"] * (1.0 - max(out[n]["spread"], base["spread"]))
    return out


def close(o, o0):
    a, b = o.float(), o0.float()
    ulp = torch.exp2(torch.floor(torch.log2(b.abs().clamp_min(1e-30))) - 7)
    return bool(((a - b).abs() <= 2 * ulp + 1e-5 * b.abs().max()).all())


def write(res, path):
    """The result as JSON with one shape per line (72 shapes of 14 timing sets each: indented, the file runs to 14 000 lines)."""
    head = {k: v for k, v in res.items() if k != "shapes"}
    with open(path, "w") as f:
        f.write(json.dumps(head)[:-1] + ', "shapes": [\n')
        f.write(",\n".join(json.dumps(r) for r in res["shapes"]))
        f.write("\n]}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--lk", default="8192,32768,65536")
    ap.add_argument("--batches", default="1,2,4,8,16,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "num_splits_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "num_splits_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    lks, batches = [int(x) for x in a.lk.split(",")], [int(x) for x in a.batches.split(",")]
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D 128, Hq 32 / Hkv 8, pack_gqa=True and without, "
                   "causal_align='bottom_right' with kv_lens drawn from [Lk / 2, Lk]; call = whole entry point, kernel = the attention entry alone "
                   "(with a split: pass 1 + pass 2 + merge); spread = range of the round medians / the figure; faster = variant < unsplit * "
                   "(1 - the larger spread)",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "shapes": []}
    for Lk in lks:
        g = torch.Generator(device=dev).manual_seed(15 + Lk)
        bmax = max(batches)
        k_all, v_all = (torch.randn(bmax, HKV, Lk, D, generator=g, device=dev, dtype=torch.bfloat16) for _ in range(2))
        q_all = torch.randn(bmax, HQ, max(LQS), D, generator=g, device=dev, dtype=torch.bfloat16)
        lens_all = torch.randint(Lk // 2, Lk + 1, (bmax,), generator=torch.Generator().manual_seed(15)).to(torch.int32)
        for B in batches:
            for Lq in LQS:
                q, k, v = q_all[:B, :, :Lq].contiguous(), k_all[:B], v_all[:B]
                lens = lens_all[:B].to(dev)
                for packed in (True, False):
                    calls, kernels, auto = variants(q, k, v, lens, Lk, packed)
                    probe, grids, outs = ctypes.c_int32(-1), {}, {}
                    for n, fn in calls.items():
                        with ops.launch_hooks(grid_probe=probe):
                            outs[n] = fn()
                        grids[n] = probe.value
                    torch.cuda.synchronize()
                    assert all(close(outs[n], outs["unsplit"]) for n in outs), "a split output left the summation-order bar"
                    assert all(close(kernels[n](), outs["unsplit"]) for n in kernels)
                    wg = B * HKV * ((HQ // HKV + 3) // 4) if packed else B * HQ
                    assert grids["unsplit"] == wg and all(grids[f"s{s}"] == wg * s for s in SPLITS) and grids["auto"] == wg * max(auto, 1), grids
                    r = {"B": B, "Lq": Lq, "Lk": Lk, "pack_gqa": packed, "workgroups_unsplit": wg, "auto_S": auto,
                         "lens_min_max": [int(lens.min()), int(lens.max())],
                         "kernel": summary(time_interleaved(kernels, a.rounds, a.reps)), "call": summary(time_interleaved(calls, a.rounds, a.reps))}
                    r["auto_ok"] = auto == 0 or (r["kernel"]["auto"]["faster"] and r["call"]["auto"]["faster"])
                    res["shapes"].append(r)
                    for what in ("kernel", "call"):
                        s = r[what]
                        line = "  ".join(f"{n} {s[n]['us']:.1f}" + (f" (x{s[n]['over_unsplit']:.2f}{'*' if s[n]['faster'] else ''})" if n != "unsplit" else
                                                                    f" (spread {s[n]['spread']:.3f})") for n in s)
                        print(f"Lk {Lk:6d} B {B:3d} Lq {Lq:2d} {'packed  ' if packed else 'unpacked'} {what:6s} auto S={auto:2d}  {line}", flush=True)
                res["auto_ok_everywhere"] = all(r["auto_ok"] for r in res["shapes"])
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                write(res, a.out)                               # (after every shape: a run cut short leaves what it measured)
        del k_all, v_all, q_all
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
