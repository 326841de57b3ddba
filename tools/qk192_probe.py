#!/usr/bin/env python3
"""First numbers of the 192-wide Q / K, 128-wide V FP8-PV route (sageattention_amd.qk192): the attention kernel alone, the whole
call (pre-pass + attention), and the two routes a caller had before it, interleaved in one run on the same inputs:

  hd256   sageattn_hd256(q, k, v zero-padded to 192)[..., :128]  (it pads all three to 256 inside the call; the pad of v to 192 is done once,
          outside the timed call, which favours this baseline)
  sdpa    torch.nn.functional.scaled_dot_product_attention(q, k, v zero-padded to 192)[..., :128]  (the same pad, outside as well)

  B2 H16 Dqk 192 Dv 128 bf16, N = 4096 and 8192 (Lq = Lk = N), causal and not.

Per (shape, variant): us = the median over the rounds of the round's median (device events around one call), spread = (max - min) / median of
the round medians, and TFLOP/s = 2 N^2 (192 + 128) B H (half of it causal) over that time -- the matrix operations the attention NEEDS, so
the padded routes are charged their time and credited no padding; for `call` the pre-pass's time is in the denominator and none of its work in
the numerator.  Every variant is warmed up at every shape before the first timed round, and the new route's output is compared with sdpa's
at every shape.  No figure is a gate.

    python tools/qk192_probe.py [--rounds 5] [--reps 10] [--out profiles/qk192_probe.json]
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

from sageattention_amd import _cabi, _cabi_qk192  # noqa: E402
from sageattention_amd.hd256 import sageattn_hd256  # noqa: E402
from sageattention_amd.qk192 import sageattn_qk192  # noqa: E402
from sageattention_amd.quant import _dims, _p, _stream  # noqa: E402

B, H, DQK, DV = 2, 16, 192, 128


def kernel_only(q, k, v, causal):
    """The attention launch alone, on images built once."""
    lib = _cabi_qk192.load()
    N, dev = q.shape[2], q.device
    nt = (N + 63) // 64
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
    f4 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    k_img, v_img, k_scale, v_scale = u8(B, H, nt, 64 * DQK), u8(B, H, nt, 64 * DV), f4(B, H, 4 * nt), f4(B, H, DV)
    k_mean = torch.empty(B, H, DQK, dtype=q.dtype, device=dev)
    ws = f4(lib.sage_qk192_ws_floats(B, H, N))
    st = lambda t: _dims(t, "HND")[4:]
    _cabi.check(lib.sage_qk192_prepass(_p(k), _p(v), _p(k_img), _p(k_scale), _p(k_mean), _p(v_img), _p(v_scale), _p(ws), ws.numel(), B, H, N, DQK, DV,
                                       *st(k), *st(v), 1, _cabi.DTYPE_BF16, _stream(q)), "sage_qk192_prepass")
    o = torch.empty_like(v)

    def run():
        _cabi.check(lib.sage_qk192_attn(_p(q), _p(k_img), _p(v_img), _p(k_scale), _p(v_scale), _p(o), None, B, H, H, N, N, DQK, DV, *st(q), *st(o),
                                        int(causal), DQK ** -0.5, _cabi.DTYPE_BF16, _stream(q)), "sage_qk192_attn")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qk192_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    variants, agree = {}, {}
    for N in (4096, 8192):
        q, k = (torch.randn(B, H, N, DQK, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
        v = torch.randn(B, H, N, DV, generator=g).to(torch.bfloat16).to(dev)
        vp = F.pad(v, (0, DQK - DV))
        for causal in (False, True):
            tag = f"N{N}_{'causal' if causal else 'full'}"
            variants[tag] = dict(
                flops=2.0 * N * N * (DQK + DV) * B * H * (0.5 if causal else 1.0),
                fns=dict(kernel=kernel_only(q, k, v, causal),
                         call=lambda q=q, k=k, v=v, c=causal: sageattn_qk192(q, k, v, is_causal=c),
                         hd256=lambda q=q, k=k, vp=vp, c=causal: sageattn_hd256(q, k, vp, is_causal=c)[..., :DV],
                         sdpa=lambda q=q, k=k, vp=vp, c=causal: F.scaled_dot_product_attention(q, k, vp, is_causal=c)[..., :DV]))
    for t, var in variants.items():             # warm-up: every variant at every shape; and what the new route computes against sdpa
        for fn in var["fns"].values():
            for _ in range(3):
                fn()
        o, r = var["fns"]["call"]().float(), var["fns"]["sdpa"]().float()
        agree[t] = dict(max_abs_diff=round((o - r).abs().max().item(), 5), max_abs_ref=round(r.abs().max().item(), 5))
    torch.cuda.synchronize()
    rounds = {(t, n): [] for t, var in variants.items() for n in var["fns"]}
    for _ in range(a.rounds):                   # interleaved: one round visits every (shape, variant)
        for t, var in variants.items():
            for n, fn in var["fns"].items():
                rounds[(t, n)].append(timed(fn, a.reps))
    out = dict(device=torch.cuda.get_device_name(0), shape=dict(B=B, H=H, Dqk=DQK, Dv=DV, dtype="bf16"), rounds=a.rounds, reps=a.reps,
               output_against_sdpa=agree, results={})
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
