"""Whole-call times of the FP8 routes on shapes whose grid does not fill the chip, in interleaved rounds on one device:
the unsplit FP8 default, the inexact split (split_kv="auto" or S), the exact split (split_kv_exact=True) and the FP16-PV default (which
splits by itself).  Shapes: the bench's decode_like call (B1 H32 Lq128 Lk32768 D128 bf16), GQA 32 / 8 at Lq in {1, 16, 128} x Lk in
{8192, 32768, 131072 + 77}, and causal B2 H32 N = 1k / 2k at S = 2 and 4.  Median over the rounds of the mean per call of each timing; per shape
also the distance of both split routes' outputs to the unsplit call's.

    python tools/split_exact_probe.py [--rounds 5] [--steps 10] [--warmup 3] [--out FILE.json]
    python tools/split_exact_probe.py --trace-exact [--steps 20]     # the exact route alone on decode_like (under rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import sageattention_amd as sa  # noqa: E402
from sageattention_amd import core  # noqa: E402


def shapes():
    yield dict(name="decode_like", B=1, Hq=32, Hkv=32, Lq=128, Lk=32768, causal=False, S=None)
    for lk in (8192, 32768, 131072 + 77):
        for lq in (1, 16, 128):
            yield dict(name=f"gqa32_8_lq{lq}_lk{lk}", B=1, Hq=32, Hkv=8, Lq=lq, Lk=lk, causal=False, S=None)
    for n in (1024, 2048):
        for s in (2, 4):
            yield dict(name=f"causal_b2_h32_n{n}_s{s}", B=2, Hq=32, Hkv=32, Lq=n, Lk=n, causal=True, S=s)


def inputs(c, dev, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(c["B"], c["Hq"], c["Lq"], 128, generator=g).to(torch.bfloat16).to(dev)
    k, v = (torch.randn(c["B"], c["Hkv"], c["Lk"], 128, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    return q, k, v


def routes(c, q, k, v):
    causal, S = c["causal"], c["S"]
    return {
        "fp8_unsplit": lambda: sa.sageattn(q, k, v, is_causal=causal),
        "fp8_split_inexact": lambda: sa.sageattn(q, k, v, is_causal=causal, split_kv="auto" if S is None else S),
        "fp8_split_exact": lambda: sa.sageattn(q, k, v, is_causal=causal, split_kv_exact=True, split_kv=S),
        "fp16_pv_default": lambda: sa.sageattn_qk_int8_pv_fp16_cuda(q, k, v, is_causal=causal),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-exact", action="store_true", help="only the exact route on decode_like, --steps calls (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace_exact:
        c = next(shapes())
        q, k, v = inputs(c, dev)
        fn = routes(c, q, k, v)["fp8_split_exact"]
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return
    res = {"what": "whole calls, us per call (median over interleaved rounds of the mean of `steps` calls), bf16, D = 128",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "shapes": {}}
    for c in shapes():
        q, k, v = inputs(c, dev)
        fns = routes(c, q, k, v)
        t = {r: [] for r in fns}
        for _ in range(a.rounds):
            for r, fn in fns.items():
                wall, _ = bench.timed(fn, a.steps, a.warmup, False, 0.0)
                t[r].append(wall / a.steps * 1e6)
        row = {"shape": {kk: c[kk] for kk in ("B", "Hq", "Hkv", "Lq", "Lk", "causal")},
               "S_exact": core._split_exact_plan(c["B"], c["Hq"], c["Lq"], c["Lk"], c["causal"], c["S"]),
               "S_inexact": core._split_kv_plan(c["B"], c["Hq"], c["Lq"], c["Lk"], c["causal"], "auto" if c["S"] is None else c["S"]),
               "us": {r: round(statistics.median(v_), 1) for r, v_ in t.items()},
               "us_all_rounds": {r: [round(x, 1) for x in v_] for r, v_ in t.items()}}
        row["exact_over_unsplit"] = round(row["us"]["fp8_split_exact"] / row["us"]["fp8_unsplit"], 3)
        # distance of the two split routes' outputs to the unsplit call's (same inputs): rel-RMS, the largest difference over max|o|, and the
        # share of elements more than 2 bf16 ulps (of the unsplit value, + 1e-5 max|o|) away -- the bar of tests/test_gpu_split_exact.py
        o0 = fns["fp8_unsplit"]().float()
        m0 = float(o0.abs().max())
        ulp = torch.exp2(torch.floor(torch.log2(o0.abs().clamp_min(1e-30))) - 7)
        for r in ("fp8_split_exact", "fp8_split_inexact"):
            d = (fns[r]().float() - o0).abs()
            row[f"{r}_vs_unsplit"] = {"rel_rms": float((d.pow(2).mean() / o0.pow(2).mean()).sqrt()), "max_abs_over_max": float(d.max()) / m0,
                                      "frac_beyond_2ulp": float((d > 2 * ulp + 1e-5 * m0).float().mean())}
        res["shapes"][c["name"]] = row
        print(c["name"], json.dumps(row["us"]), "exact/unsplit", row["exact_over_unsplit"],
              "vs unsplit: exact", row["fp8_split_exact_vs_unsplit"], "inexact", row["fp8_split_inexact_vs_unsplit"], flush=True)
        del q, k, v, fns
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
