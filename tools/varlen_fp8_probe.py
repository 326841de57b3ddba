"""FP8 PV vs FP16 PV on packed batches: the C4 shape (bench.C4_LENS, Hq 32, Hkv 8, D 128, bf16) through sageattn_qk_int8_pv_fp8_varlen and
sageattn_varlen, causal and non-causal, the attention kernel alone (operands prepared once) and the whole call.  TFLOP/s as bench.py counts
C4: sum over the sequences of 4 Hq L^2 D, halved when causal.

    python tools/varlen_fp8_probe.py [--steps 40] [--warmup 10] [--ramp 0.5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import sageattention_amd as sa  # noqa: E402
from sageattention_amd import core  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ramp", type=float, default=0.5, help="seconds of untimed work in front of every timing (clock ramp)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lens = bench.C4_LENS
    g = torch.Generator(device="cpu").manual_seed(4)          # bench.py's C4 inputs
    total = sum(lens)
    q = torch.randn(total, 32, 128, generator=g).to(torch.bfloat16).to(dev)
    k = torch.randn(total, 8, 128, generator=g).to(torch.bfloat16).to(dev)
    v = torch.randn(total, 8, 128, generator=g).to(torch.bfloat16).to(dev)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev)
    L = max(lens)
    res = {"workload": f"C4: Hq=32 Hkv=8 D=128 bf16, lengths {lens}", "device": torch.cuda.get_device_name(0),
           "steps": a.steps, "warmup": a.warmup}
    for causal in (True, False):
        fl = sum(4.0 * 32 * n * n * 128 for n in lens) / (2 if causal else 1)
        row = {}
        for route in ("fp16", "fp8"):
            if route == "fp8":
                st = core._varlen_prepare(q, k, v, cu, cu, L, L, causal, None, True, {}, v_fp8=True)
                kern = lambda: core._varlen_attend_f8(st, True, False)
                call = lambda: sa.sageattn_qk_int8_pv_fp8_varlen(q, k, v, cu, cu, L, L, is_causal=causal)
            else:
                st = core._varlen_prepare(q, k, v, cu, cu, L, L, causal, None, True, {})
                kern = lambda: core._varlen_attend(st)
                call = lambda: sa.sageattn_varlen(q, k, v, cu, cu, L, L, is_causal=causal)
            _, dev_k = bench.timed(kern, a.steps, a.warmup, False, a.ramp)
            kern_ms = sum(dev_k) / len(dev_k)
            wall, _ = bench.timed(call, a.steps, a.warmup, False, a.ramp)
            call_ms = wall * 1e3 / a.steps                       # (seconds -> ms per call)
            row[route] = {"kernel_only": {"ms": round(kern_ms, 4), "tflops": round(fl / kern_ms / 1e9, 1)},
                          "whole_call": {"ms": round(call_ms, 4), "tflops": round(fl / call_ms / 1e9, 1)}}
        row["fp8_over_fp16"] = {p: round(row["fp16"][p]["ms"] / row["fp8"][p]["ms"], 3) for p in ("kernel_only", "whole_call")}
        res["causal" if causal else "non_causal"] = row
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
