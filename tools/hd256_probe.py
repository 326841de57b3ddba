#!/usr/bin/env python3
"""First numbers of the head_dim = 256 FP8-PV route (sageattention_amd.hd256): the attention kernel alone, the whole call
(pre-pass + attention) and torch.nn.functional.scaled_dot_product_attention on the same inputs, interleaved in one run.

  B2 H16 D256 bf16, N = 4096 and 8192 (Lq = Lk = N), causal and not.

Per (shape, variant): us = the median over the rounds of the round's median (device events around one call), spread = (max - min) / median of
the round medians, and TFLOP/s = 4 N^2 D B H (half of it causal) over that time -- the matrix operations of the attention itself, whatever
their format; for `call` the pre-pass's time is in the denominator and none of its work in the numerator.  Every variant is warmed up at
every shape before the first timed round.  No figure is a gate.

    python tools/hd256_probe.py [--rounds 5] [--reps 10] [--out profiles/hd256_probe.json]
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

from sageattention_amd import _cabi, _cabi_hd256  # noqa: E402
from sageattention_amd.hd256 import sageattn_hd256  # noqa: E402
from sageattention_amd.quant import _dims, _p, _stream  # noqa: E402

B, H, D = 2, 16, 256


def kernel_only(q, k, v, causal):
    """The attention launch alone, on images built once."""
    lib = _cabi_hd256.load()
    N, dev = q.shape[2], q.device
    nt = (N + 63) // 64
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
    f4 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    k_img, v_img, k_scale, v_scale, k_mean = u8(B, H, nt, 64 * D), u8(B, H, nt, 64 * D), f4(B, H, 4 * nt), f4(B, H, D), torch.empty(B, H, D, dtype=q.dtype, device=dev)
    ws = f4(lib.sage_hd256_ws_floats(B, H, N))
    st = lambda t: _dims(t, "HND")[4:]
    _cabi.check(lib.sage_hd256_prepass(_p(k), _p(v), _p(k_img), _p(k_scale), _p(k_mean), _p(v_img), _p(v_scale), _p(ws), ws.numel(), B, H, N, D,
                                       *st(k), *st(v), 1, _cabi.DTYPE_BF16, _stream(q)), "sage_hd256_prepass")
    o = torch.empty_like(q)

    def run():
        _cabi.check(lib.sage_hd256_attn(_p(q), _p(k_img), _p(v_img), _p(k_scale), _p(v_scale), _p(o), None, B, H, H, N, N, D, *st(q), *st(o),
                                        int(causal), D ** -0.5, _cabi.DTYPE_BF16, _stream(q)), "sage_hd256_attn")
    run.keep = (k_img, v_img, k_scale, v_scale, k_mean, ws, o)
    return run


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hd256_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    variants = {}
    for N in (4096, 8192):
        q, k, v = (torch.randn(B, H, N, D, generator=g).to(torch.bfloat16).to(dev) for _ in range(3))
        for causal in (False, True):
            tag = f"N{N}_{'causal' if causal else 'full'}"
            variants[tag] = dict(
                flops=4.0 * N * N * D * B * H * (0.5 if causal else 1.0),
                fns=dict(kernel=kernel_only(q, k, v, causal),
                         call=lambda q=q, k=k, v=v, c=causal: sageattn_hd256(q, k, v, is_causal=c),
                         sdpa=lambda q=q, k=k, v=v, c=causal: F.scaled_dot_product_attention(q, k, v, is_causal=c)))
    for var in variants.values():               # warm-up: every variant at every shape
        for fn in var["fns"].values():
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    rounds = {(t, n): [] for t, var in variants.items() for n in var["fns"]}
    for _ in range(a.rounds):                   # interleaved: one round visits every (shape, variant)
        for t, var in variants.items():
            for n, fn in var["fns"].items():
                rounds[(t, n)].append(timed(fn, a.reps))
    out = dict(device=torch.cuda.get_device_name(0), shape=dict(B=B, H=H, D=D, dtype="bf16"), rounds=a.rounds, reps=a.reps, results={})
    for (t, n), meds in rounds.items():
        us = statistics.median(meds)
        out["results"].setdefault(t, {})[n] = dict(us=round(us, 1), spread=round((max(meds) - min(meds)) / us, 4),
                                                   tflops=round(variants[t]["flops"] / us * 1e-6, 1), round_medians_us=[round(m, 1) for m in meds])
        print(f"{t:14s} {n:7s} {us:9.1f} us  spread {out['results'][t][n]['spread']:.3f}  {out['results'][t][n]['tflops']:7.1f} TFLOP/s")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
