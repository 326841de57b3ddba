#!/usr/bin/env python3
"""What a sliding window (window_size=(W - 1, 0)) buys on the FP8-PV route, and what its flag costs: whole calls and the attention kernel
alone, interleaved.

  long causal     B2 H32 D128 bf16, Lq = Lk = 8192, is_causal=True:
                    plain        no keyword (the default causal kernels)
                    qstart0      q_start = 0 (the q_start kernels: the route a window rides on, without one)
                    w_none       W = Lk + Lq: the WINDOW kernels with a window that cuts no row -- the flag's cost
                    w4096, w1024, w256
  chunked prefill B2 H32 D128 bf16, Lq 512 new rows against Lk 8192, lens drawn as tools/q_start_probe.py draws them, bottom-right:
                    br_aligned / br_unaligned           (no window: q_start_probe's lines)
                    br_aligned_w1024 / br_unaligned_w1024

Per variant: us (median over the rounds of the round's median, device events), spread of the round medians, the ratio to the variant without
a window, ps per attended (row, key) pair, and the 64-key tiles a work item runs on average -- counted by a restatement of the kernel's
geometry, the expectation the time is compared with: `expected_us` = the unwindowed kernel's time scaled by the tile counts,
`gap_us_per_item` = (us - expected_us) * resident workgroups / work items, what a windowed work item costs beyond its tiles (the head tiles'
general form and the second priming of the ring).

    python tools/window_probe.py [--rounds 5] [--reps 10] [--out profiles/window_probe.json]
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

D, B, H = 128, 2, 32
UNALIGN = 23
RESIDENT = 512          # workgroups a 256-CU device holds of the D = 128 kernels (two per CU)


def item_tiles(Lq, Lk, n, s, W, qblk):
    """64-key tiles the work item of query block ``qblk`` runs (W = 0: no window): the kernel's loop bounds, restated."""
    n = max(0, min(n, Lk))
    kc0 = 0
    if W:
        a0 = s - W + 128 * qblk + 1
        kc0 = (a0 // 64) * 64 if a0 > 0 else 0
    keys = max(0, n - kc0)
    lim = max(0, -(-(128 * qblk + 128 + s - kc0) // 64))
    return min(lim, -(-keys // 64))


def mean_tiles(Lq, Lk, lens, starts, W):
    items = [(n, s, qb) for n, s in zip(lens, starts) for qb in range(-(-Lq // 128))]
    return sum(item_tiles(Lq, Lk, n, s, W, qb) for n, s, qb in items) / len(items)


def pairs(Lq, lens, starts, W):
    """(row, key) pairs attended per head, summed over the samples."""
    tot = 0
    for n, s in zip(lens, starts):
        for i in range(Lq):
            lo, hi = max(0, s + i - W + 1) if W else 0, min(n - 1, s + i)
            tot += max(0, hi - lo + 1)
    return tot


def build(dev):
    g = torch.Generator(device="cpu").manual_seed(11)
    mk = lambda L: torch.randn(B, H, L, D, generator=g).to(torch.bfloat16).to(dev)
    sm = core._sm_log2(D ** -0.5)
    out = {}
    # ---- long causal
    N = 8192
    q, k, v = mk(N), mk(N), mk(N)
    _, _, k8, ks, vimg, vs, _ = core._prepass_kv(q, k, v, "HND", "per_thread", 64, True, False, False, core._fused_prepass_wanted(k, "HND", None))
    full, zero = torch.full((B,), N, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    spec = {"plain": None, "qstart0": 0, "w_none": 2 * N, "w4096": 4096, "w1024": 1024, "w256": 256}
    calls, kernels, meta = {}, {}, {}
    for name, W in spec.items():
        kw = {} if W is None else dict(q_start=0) if W == 0 else dict(window_size=(W - 1, 0))
        calls[name] = lambda kw=kw: sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=True, pv_accum_dtype="fp32+fp32", **kw)
        if W is None:
            kernels[name] = lambda: core._attn_fused_q(q, k8, vimg, vs, ks, "HND", True, sm, False)
        else:
            kernels[name] = lambda W=W: core._attn_fused_q(q, k8, vimg, vs, ks, "HND", True, sm, False, kv_lens=full, q_start=zero, window=W)
        Wm = 0 if not W or W >= 2 * N else W
        meta[name] = dict(pairs=H * pairs(N, [N] * B, [0] * B, Wm), tiles=mean_tiles(N, N, [N] * B, [0] * B, Wm), items=B * H * (N // 128))
    out["long_causal"] = dict(shape=dict(B=B, H=H, Lq=N, Lk=N), calls=calls, kernels=kernels, meta=meta, base="plain", keep=(q, k, v, k8, ks, vimg, vs))
    # ---- chunked prefill
    Lq, Lk = 512, 8192
    q2, k2, v2 = mk(Lq), mk(Lk), mk(Lk)
    drawn = 64 * torch.randint(Lk // 128, Lk // 64 + 1, (B,), generator=g)
    calls, kernels, meta = {}, {}, {}
    for tag, lens_h in (("br_aligned", [int(x) for x in drawn]), ("br_unaligned", [int(x) - UNALIGN for x in drawn])):
        lens = torch.tensor(lens_h, dtype=torch.int32, device=dev)
        _, _, k8b, ksb, vimgb, vsb, _ = core._prepass_kv(q2, k2, v2, "HND", "per_thread", 64, True, False, False, False, kv_lens=lens)
        qs = core._q_start_tensor(None, lens, B, Lq, Lk, dev)
        starts = [n - Lq for n in lens_h]
        for W in (0, 1024):
            name = tag + (f"_w{W}" if W else "")
            kw = dict(window_size=(W - 1, 0)) if W else {}
            calls[name] = lambda lens=lens, kw=kw: sa.sageattn_qk_int8_pv_fp8_cuda(q2, k2, v2, is_causal=True, pv_accum_dtype="fp32+fp32", kv_lens=lens,
                                                                                   causal_align="bottom_right", **kw)
            kernels[name] = lambda a=(k8b, ksb, vimgb, vsb, lens, qs), W=W: core._attn_fused_q(q2, a[0], a[2], a[3], a[1], "HND", True, sm, False,
                                                                                               kv_lens=a[4], q_start=a[5], window=W)
            meta[name] = dict(pairs=H * pairs(Lq, lens_h, starts, W), tiles=mean_tiles(Lq, Lk, lens_h, starts, W), items=B * H * (Lq // 128), lens=lens_h)
    out["chunked_prefill"] = dict(shape=dict(B=B, H=H, Lq=Lq, Lk=Lk), calls=calls, kernels=kernels, meta=meta, base=None, keep=(q2, k2, v2))
    return out


def time_interleaved(fns, rounds, reps):
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


def summary(per_round, meta, base_of):
    out = {}
    for n, xs in per_round.items():
        med = statistics.median(xs)
        out[n] = {"us": round(med, 1), "spread": round((max(xs) - min(xs)) / med, 4), "us_rounds": [round(x, 1) for x in xs],
                  "ps_per_row_key_pair": round(med * 1e6 / meta[n]["pairs"], 4) if meta[n]["pairs"] else None,
                  "tiles_per_item": round(meta[n]["tiles"], 2)}
    for n in out:
        b = base_of(n)
        out[n]["over_no_window"] = round(out[n]["us"] / out[b]["us"], 4)
        exp = out[b]["us"] * meta[n]["tiles"] / meta[b]["tiles"]
        out[n]["expected_us"] = round(exp, 1)
        out[n]["gap_us_per_item"] = round((out[n]["us"] - exp) * RESIDENT / meta[n]["items"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "window_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    groups = build(dev)
    lc = groups["long_causal"]["calls"]
    assert torch.equal(lc["plain"](), lc["w_none"]()), "a window that cuts no row must be the plain causal call, bit for bit"
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D = 128, causal; call = whole entry "
                   "point, kernel = attention launch alone; spread = range of the round medians / the figure; over_no_window = the figure over the "
                   "same shape's variant without a window; tiles_per_item = 64-key tiles a work item runs on average (the kernel's loop bounds); "
                   "expected_us = the unwindowed figure scaled by the tile counts; gap_us_per_item = (us - expected_us) * 512 resident "
                   "workgroups / work items",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps}
    for gname, grp in groups.items():
        base_of = (lambda n: "plain") if grp["base"] else (lambda n: n.split("_w")[0])
        r = {"shape": grp["shape"], "attended_row_key_pairs": {n: m["pairs"] for n, m in grp["meta"].items()}}
        if gname == "chunked_prefill":
            r["lens"] = {n: m["lens"] for n, m in grp["meta"].items()}
        for what in ("call", "kernel"):
            r[what] = summary(time_interleaved(grp[what + "s"], a.rounds, a.reps), grp["meta"], base_of)
            print(gname, what, flush=True)
            for n, x in r[what].items():
                print(f"  {n:20s} {x['us']:9.1f} us (spread {x['spread']:.3f})  x{x['over_no_window']:.4f}  {x['ps_per_row_key_pair']} ps/pair  "
                      f"{x['tiles_per_item']:6.2f} tiles/item  expected {x['expected_us']:9.1f} us  gap {x['gap_us_per_item']:+.3f} us/item", flush=True)
        res[gname] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
