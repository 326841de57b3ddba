#!/usr/bin/env python3
"""First numbers of the packed 192-wide Q / K, 128-wide V FP8-PV route (sageattention_amd.qk192_varlen): the attention kernel
alone and the whole call (plan + pre-pass + attention), against the only route a caller had before it, interleaved in one run on the same inputs.

  bf16, Hq 16 / Hkv 16, Dqk 192, Dv 128, causal bottom-right:
    equal8   eight sequences of 4096 rows and keys
    mix      256 .. 16384 rows and keys, 32512 in all
    chunks   four chunks of 512 rows against prefixes of 4096 / 8192 keys (Lk_s = prefix + 512)
  loop_call / loop_kernel   a Python loop of sageattn_qk192 over the sequences (equal8, mix: Lq_s = Lk_s, so its top-left mask is the same
                            mask) / the loop's attention launches alone on images built once
  sdpa_loop                 chunks, which the dense call cannot express: scaled_dot_product_attention per sequence with a causal_lower_right
                            bias and v zero-padded to 192 (the pad outside the timed call)

Per (shape, variant): us = the median over the rounds of the round's median (device events around one whole call or loop), spread = (max - min)
/ median of the round medians.  Every variant is warmed up at every shape before the first timed round.  No figure is a gate.

    python tools/qk192_varlen_probe.py [--rounds 5] [--reps 10] [--out profiles/qk192_varlen_probe.json]
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
from torch.nn.attention.bias import causal_lower_right  # noqa: E402

from sageattention_amd import _cabi, _cabi_qk192, _cabi_qk192v  # noqa: E402
from sageattention_amd.qk192 import sageattn_qk192  # noqa: E402
from sageattention_amd.qk192_varlen import sageattn_qk192_varlen, size_bounds  # noqa: E402
from sageattention_amd.quant import _dims, _p, _stream  # noqa: E402

H, DQK, DV = 16, 192, 128
SHAPES = dict(equal8=[(4096, 4096)] * 8,
              mix=[(n, n) for n in (256, 512, 1024, 2048, 4096, 8192, 16384)],
              chunks=[(512, 4096 + 512), (512, 8192 + 512)] * 2)
BF16 = _cabi.DTYPE_BF16


def packed_kernel(q, k, v, cu_q, cu_k):
    """The packed attention launch alone, on a plan and images built once."""
    lib, dev, nseq = _cabi_qk192v.load(), q.device, cu_q.numel() - 1
    tq, tk = q.shape[0], k.shape[0]
    tiles = size_bounds(tq, tk, nseq)[1]
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
    f4 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    k_img, v_img, k_scale, v_scale = u8(H, tiles, 64 * DQK), u8(H, tiles, 64 * DV), f4(H, 4 * tiles), f4(nseq, H, DV)
    k_mean, nb = torch.empty(nseq, H, DQK, dtype=q.dtype, device=dev), lib.sage_qk192v_ws_bytes(nseq, H, tq, tk)
    ws, o = u8(nb), torch.empty(tq, H, DV, dtype=q.dtype, device=dev)
    _cabi.check(lib.sage_qk192v_prepass(_p(k), _p(v), _p(cu_q), _p(cu_k), _p(k_img), _p(k_scale), _p(k_mean), _p(v_img), _p(v_scale), _p(ws), nb, nseq,
                                        tq, tk, H, H, DQK, DV, k.stride(0), k.stride(1), v.stride(0), v.stride(1), 2, 1, BF16, _stream(q)), "prepass")

    def run():
        _cabi.check(lib.sage_qk192v_attn(_p(q), _p(cu_q), _p(cu_k), _p(k_img), _p(v_img), _p(k_scale), _p(v_scale), _p(ws), nb, _p(o), None, nseq, tq, tk,
                                         H, H, DQK, DV, q.stride(0), q.stride(1), o.stride(0), o.stride(1), 2, DQK ** -0.5, BF16, _stream(q)), "attn")
    run.keep = (k_img, v_img, k_scale, v_scale, k_mean, ws, o)
    return run


def dense_kernel(q, k, v):
    """One sequence's dense attention launch alone (NHD, B = 1, causal), on images built once."""
    lib, dev, (Lq, Lk) = _cabi_qk192.load(), q.device, (q.shape[1], k.shape[1])
    nt = (Lk + 63) // 64
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
    f4 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    k_img, v_img, k_scale, v_scale = u8(1, H, nt, 64 * DQK), u8(1, H, nt, 64 * DV), f4(1, H, 4 * nt), f4(1, H, DV)
    k_mean, ws = torch.empty(1, H, DQK, dtype=q.dtype, device=dev), f4(lib.sage_qk192_ws_floats(1, H, Lk))
    st = lambda t: _dims(t, "NHD")[4:]
    _cabi.check(lib.sage_qk192_prepass(_p(k), _p(v), _p(k_img), _p(k_scale), _p(k_mean), _p(v_img), _p(v_scale), _p(ws), ws.numel(), 1, H, Lk, DQK, DV,
                                       *st(k), *st(v), 1, BF16, _stream(q)), "sage_qk192_prepass")
    o = torch.empty(1, Lq, H, DV, dtype=q.dtype, device=dev)

    def run():
        _cabi.check(lib.sage_qk192_attn(_p(q), _p(k_img), _p(v_img), _p(k_scale), _p(v_scale), _p(o), None, 1, H, H, Lq, Lk, DQK, DV, *st(q), *st(o),
                                        1, DQK ** -0.5, BF16, _stream(q)), "sage_qk192_attn")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qk192_varlen_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    variants = {}
    for tag, seqs in SHAPES.items():
        tq, tk = sum(s[0] for s in seqs), sum(s[1] for s in seqs)
        q, k = (torch.randn(n, H, DQK, generator=g).to(torch.bfloat16).to(dev) for n in (tq, tk))
        v = torch.randn(tk, H, DV, generator=g).to(torch.bfloat16).to(dev)
        cu = lambda i: torch.tensor([0] + [s[i] for s in seqs]).cumsum(0).to(torch.int32).to(dev)
        cu_q, cu_k, mq, mk = cu(0), cu(1), max(s[0] for s in seqs), max(s[1] for s in seqs)
        oq, ok = [0] + list(cu_q.tolist()[1:]), [0] + list(cu_k.tolist()[1:])
        sl = [(q[oq[i]:oq[i + 1]][None], k[ok[i]:ok[i + 1]][None], v[ok[i]:ok[i + 1]][None]) for i in range(len(seqs))]
        fns = dict(kernel=packed_kernel(q, k, v, cu_q, cu_k),
                   call=lambda q=q, k=k, v=v, cu_q=cu_q, cu_k=cu_k, mq=mq, mk=mk: sageattn_qk192_varlen(q, k, v, cu_q, cu_k, mq, mk, is_causal=True))
        if tag != "chunks":
            dk = [dense_kernel(*s) for s in sl]
            fns["loop_kernel"] = lambda dk=dk: [f() for f in dk]
            fns["loop_call"] = lambda sl=sl: [sageattn_qk192(a_, b_, c_, tensor_layout="NHD", is_causal=True) for a_, b_, c_ in sl]
        else:
            sd = [(a_.transpose(1, 2), b_.transpose(1, 2), F.pad(c_, (0, DQK - DV)).transpose(1, 2)) for a_, b_, c_ in sl]
            fns["sdpa_loop"] = lambda sd=sd: [F.scaled_dot_product_attention(a_, b_, c_, attn_mask=causal_lower_right(a_.shape[2], b_.shape[2]))[..., :DV]
                                              for a_, b_, c_ in sd]
        variants[tag] = dict(fns=fns, tokens=dict(total_q=tq, total_k=tk, nseq=len(seqs)))
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
    out = dict(device=torch.cuda.get_device_name(0), shape=dict(Hq=H, Hkv=H, Dqk=DQK, Dv=DV, dtype="bf16", mask="causal bottom-right"),
               rounds=a.rounds, reps=a.reps, shapes={t: var["tokens"] for t, var in variants.items()}, results={})
    for (t, n), meds in rounds.items():
        us = statistics.median(meds)
        out["results"].setdefault(t, {})[n] = dict(us=round(us, 1), spread=round((max(meds) - min(meds)) / us, 4), round_medians_us=[round(m, 1) for m in meds])
        print(f"{t:8s} {n:12s} {us:10.1f} us  spread {out['results'][t][n]['spread']:.3f}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
