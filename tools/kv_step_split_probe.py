#!/usr/bin/env python3
"""What the split step call buys against the listed step call and costs against the dense split call (sageattention_amd.paged_kv_list_split,
DESIGN.md 3.25).

Method of tools/kv_step_probe.py: bf16, D 128, Hq 32 / Hkv 8, pages of 256 keys, the table a random permutation; per round every variant is
warmed, then timed call by call with device events; a figure is the median over the interleaved rounds of the round's median, "spread" the
range of the round medians relative to it.  Bits are checked before anything is timed: the new call against the dense split call at the same S
(decode rows) and against the listed call (chunk rows).

  decode   pure decode steps: B 1 / 4 / 8 sequences of one row at capacity Lk 8192 / 32768 / 65536 with lengths in [Lk / 2, Lk]:
           listed          sageattn_kvcache_step_listed(q, cache, cu, 1)                      -- the parent's call
           split_S         sageattn_kvcache_step_split(q, cache, cu, 1, S), S 8 / 16 / 32 / "auto" (auto_S: what the plan chose, 0 = the listed call)
           dense_S         sageattn_kvcache_split(q [B, 1, Hq, D], cache, S, pack_gqa=True), bottom-right, the same S
  serving  a serving-shaped cache: capacity 65536, contexts of 8192, B 4, S 32 / 64 -- most chunks are empty
  mixed    four decode sequences of 32768 keys plus two chunks of 512 rows (capacity 32768): listed, split_8 / 16 / 32
No ratio here is an acceptance bar.

    python tools/kv_step_split_probe.py [--rounds 5] [--reps 10] [--out profiles/kv_step_split_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from kv_step_probe import _nothing  # noqa: E402
from kv_varlen_probe import D, HKV, HQ, PAGE, _view, time_interleaved  # noqa: E402
from sageattention_amd import core  # noqa: E402
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache  # noqa: E402
from sageattention_amd.paged_kv_list import sageattn_kvcache_step_listed  # noqa: E402
from sageattention_amd.paged_kv_list_split import sageattn_kvcache_step_split  # noqa: E402
from sageattention_amd.paged_kv_split import sageattn_kvcache_split  # noqa: E402

BR = dict(tensor_layout="NHD", is_causal=True, causal_align="bottom_right", pack_gqa=True)


def _filled(counts, ctx, cap, seed, dev):
    """A cache of capacity ``cap`` with contexts ``ctx`` (the step's rows included), the packed queries and their prefix array.  One sequence's
    content is drawn and repeated: what is timed does not depend on it."""
    B, max_pages = len(counts), cap // PAGE
    g = torch.Generator(device=dev).manual_seed(seed)
    k0, v0 = (torch.randn(1, HKV, max(ctx), D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(2))
    c = PagedQuantizedKVCache.allocate(2 * B * max_pages, PAGE, B, max_pages, HKV, D, torch.bfloat16, dev)
    c.block_table.copy_(torch.randperm(2 * B * max_pages, generator=torch.Generator().manual_seed(seed))[:B * max_pages].to(torch.int32).to(dev).view(B, max_pages))
    c.seed(k0.float().mean(dim=2).to(k0.dtype).repeat(B, 1, 1), (v0.abs().float().amax(dim=2) * 2.0).repeat(B, 1, 1))
    c.append(k0.repeat(B, 1, 1, 1), v0.repeat(B, 1, 1, 1), torch.tensor(ctx, dtype=torch.int32, device=dev))
    assert c.lens.tolist() == list(ctx)
    cu = torch.tensor([sum(counts[:b]) for b in range(B + 1)], dtype=torch.int32, device=dev)
    q = torch.randn(sum(counts), HQ, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    return c, q, cu


def _same(a, b, what):
    assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), what


def decode(B, cap, ctx, splits, dev, seed):
    c, q, cu = _filled([1] * B, ctx, cap, seed, dev)
    qd = q.view(B, 1, HQ, D)
    fns = {"listed": lambda: sageattn_kvcache_step_listed(q, c, cu, 1)}
    auto = core._num_splits_plan(B, HQ, HKV, 1, cap, True)
    for S in splits:
        fns[f"split_{S}"] = (lambda S=S: sageattn_kvcache_step_split(q, c, cu, 1, S))
        if S != "auto":
            fns[f"dense_{S}"] = (lambda S=S: sageattn_kvcache_split(qd, c, S, **BR))
            _same(fns[f"split_{S}"](), fns[f"dense_{S}"]().view(B, HQ, D), f"split_{S} != dense_{S}")
    if "auto" in splits:
        _same(fns["split_auto"](), sageattn_kvcache_step_split(q, c, cu, 1, auto) if auto else fns["listed"](), "auto")
    assert bool(torch.isfinite(fns["listed"]().float()).all())
    return {n: (_nothing, f) for n, f in fns.items()}, auto


def mixed(dev):
    cap, counts = 32768, [1, 1, 1, 1, 512, 512]
    c, q, cu = _filled(counts, [32768, 30000, 28000, 32768, 8192, 4096], cap, 5, dev)
    fns = {"listed": lambda: sageattn_kvcache_step_listed(q, c, cu, 512)}
    for S in (8, 16, 32):
        fns[f"split_{S}"] = (lambda S=S: sageattn_kvcache_step_split(q, c, cu, 512, S))
        o = fns[f"split_{S}"]()
        _same(o[4:], fns["listed"]()[4:], f"split_{S}: chunk rows != listed")
        _same(o[:4], sageattn_kvcache_split(q[:4].view(4, 1, HQ, D), _view(c, 0, 4), S, **BR).view(4, HQ, D), f"split_{S}: decode rows != dense")
    return {n: (_nothing, f) for n, f in fns.items()}, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_step_split_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kv_step_split_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D 128, Hq 32 / Hkv 8, pages of 256 keys.  decode: B "
                   "sequences of one row, lengths in [Lk / 2, Lk] at capacity Lk; listed = sageattn_kvcache_step_listed (the parent's call), split_S = "
                   "sageattn_kvcache_step_split with num_splits S, dense_S = sageattn_kvcache_split(pack_gqa=True) on a dense q at the same S; auto_S = what "
                   "core._num_splits_plan chose (0: the listed call).  serving: capacity 65536, contexts of 8192.  mixed: four decode sequences of about 32768 "
                   "keys plus two chunks of 512 rows.  spread = range of the round medians / the figure; x_over_y = ratio of the figures of the same run",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "decode": [], "serving": [], "mixed": []}

    def run(kind, tag, fns, auto):
        per_round = time_interleaved(fns, a.rounds, a.reps)
        r = dict(tag, auto_S=auto)
        for n, xs in per_round.items():
            med = statistics.median(xs)
            r[n] = {"us": round(med, 1), "spread": round((max(xs) - min(xs)) / med, 4), "us_rounds": [round(x, 1) for x in xs]}
        for n in fns:
            if n.startswith("split_"):
                r[f"{n}_over_listed"] = round(r[n]["us"] / r["listed"]["us"], 4)
                d = "dense_" + n[6:]
                if d in r:
                    r[f"{n}_over_{d}"] = round(r[n]["us"] / r[d]["us"], 4)
        res[kind].append(r)
        print(f"{kind} {tag} auto {auto}: " + "  ".join(f"{n} {r[n]['us']:8.1f} us (+-{100 * r[n]['spread']:.1f}%)" for n in fns), flush=True)
        print("    " + "  ".join(f"{k} x{v:.3f}" for k, v in r.items() if "_over_" in k), flush=True)

    for cap in (8192, 32768, 65536):
        for B in (1, 4, 8):
            g = torch.Generator().manual_seed(cap + B)
            ctx = [cap] + [int(x) for x in torch.randint(cap // 2, cap + 1, (B - 1,), generator=g)]
            fns, auto = decode(B, cap, ctx, (8, 16, 32, "auto"), dev, cap + B)
            run("decode", {"Lk": cap, "B": B, "contexts": ctx}, fns, auto)
            del fns
            torch.cuda.empty_cache()
    fns, auto = decode(4, 65536, [8192] * 4, (32, 64), dev, 9)
    run("serving", {"Lk": 65536, "B": 4, "contexts": [8192] * 4}, fns, auto)
    del fns
    torch.cuda.empty_cache()
    fns, auto = mixed(dev)
    run("mixed", {"Lk": 32768, "counts": [1, 1, 1, 1, 512, 512]}, fns, auto)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
