#!/usr/bin/env python3
"""What a fork of the paged quantised KV cache costs and what sharing pages does to a decode step (PagedQuantizedKVCache.fork).

Shapes (those of tools/paged_kv_probe.py): bf16, D 128, Hq 32 / Hkv 8, a context of 8192 keys, pages of 256 keys.  Every parent holds 8092 keys:
31 whole pages and an open page of 156 keys (three tiles to copy), in a table of 33 entries.

1  "fork_N" against "refill_N", N = 1 / 8 / 32 sequences made out of N parents in one cache of 2 N slots:
     fork_N     cache.fork(parents, children, new pages)                                       -- one launch, no raw rows
     refill_N   cache.seed(k_mean, v_amax, slots=children) + cache.append(the 8092 raw rows)    -- what a caller does without fork
   Before anything is timed, attention on the children is compared with attention on the parents bit for bit, after either.
2  One decode step (append one row + sageattn_kvcache, Lq 1, causal_align="bottom_right", pack_gqa=True) and the attention call alone, of 32
   sequences with the same 8092 keys:
     shared_*   31 forks of one parent: the 31 whole pages are the same pages for all 32, the last page is each sequence's own
     private_*  every sequence in pages of its own
     contig_*   the contiguous QuantizedKVCache (its round spread is the yardstick for the other two)
   The outputs of all three are compared bit for bit before anything is timed; before every timed step the lengths are put back, outside
   the timed interval.

Per round every variant is warmed, then timed call by call with device events; the figure of a variant is the median over the rounds of the
round's median, "spread" the range of the round medians relative to it.

    python tools/kv_fork_probe.py [--rounds 5] [--reps 10] [--out profiles/kv_fork_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache  # noqa: E402
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache  # noqa: E402

HQ, HKV, D, PAGE = 32, 8, 128, 256
LEN, MAX_PAGES = 8092, 33                  # 31 whole pages + 156 keys; room for one page more
FORKS, SHARERS = (1, 8, 32), 32
KW = dict(is_causal=True, causal_align="bottom_right", pack_gqa=True)
OWNED = (LEN + PAGE - 1) // PAGE           # 32 pages per parent


def _stats(k, v):
    return k.float().mean(dim=2).to(k.dtype), v.abs().float().amax(dim=2) * 2.0


def fork_variants(k, v, q, n):
    """{name: (untimed setup, timed call)}: ``n`` parents in slots 0 .. n - 1 of a cache of 2 n slots, children in slots n .. 2 n - 1"""
    dev = k.device
    km, va = _stats(k[:n], v[:n])
    c = PagedQuantizedKVCache.allocate(2 * n * MAX_PAGES, PAGE, 2 * n, MAX_PAGES, HKV, D, k.dtype, dev)
    perm = torch.randperm(2 * n * MAX_PAGES, generator=torch.Generator().manual_seed(n)).to(torch.int32).to(dev)
    table = perm.view(2 * n, MAX_PAGES).clone()
    c.block_table.copy_(table)
    c.seed(km.repeat(2, 1, 1), va.repeat(2, 1, 1))
    rows_k, rows_v = k[:n].repeat(2, 1, 1, 1), v[:n].repeat(2, 1, 1, 1)
    c.append(rows_k, rows_v, torch.tensor([LEN] * n + [0] * n, dtype=torch.int32, device=dev))
    src = torch.arange(n, dtype=torch.int32, device=dev)
    dst = src + n
    new = table[n:, OWNED - 1].contiguous()            # the page the child's own row names where the open page goes: free, nobody else names it
    child_lens = torch.tensor([0] * n + [LEN] * n, dtype=torch.int32, device=dev)
    slots = list(range(n, 2 * n))
    qq = q[:n].repeat(2, 1, 1, 1)

    def nothing():
        pass

    def restore():                                   # (a fork rewrote the children's rows: give them their own pages back)
        c.block_table.copy_(table)

    def fork():
        c.fork(src, dst, new)

    def refill():
        c.seed(km, va, slots=slots)
        c.append(rows_k, rows_v, child_lens)

    for fn, before in ((fork, nothing), (refill, restore)):
        c.lens[n:] = 0
        before()
        fn()
        o, lse = sageattn_kvcache(qq, c, return_lse=True, **KW)
        assert torch.equal(c.lens[n:], c.lens[:n]) and int(c.lens[0]) == LEN
        assert torch.equal(o[n:], o[:n]) and torch.equal(lse[n:], lse[:n]), f"{fn.__name__}: a child must attend as its parent, bit for bit"
        assert bool(torch.isfinite(o.float()).all())
    return {f"fork_{n}": (nothing, fork), f"refill_{n}": (restore, refill)}


def step_variants(k, v, q):
    """{name: (untimed setup, timed call)}: SHARERS sequences with the keys of ``k[0]``, one row ``k[b, :, LEN]`` appended per step"""
    dev, B = k.device, SHARERS
    km, va = _stats(k[:1], v[:1])
    km, va = km.repeat(B, 1, 1), va.repeat(B, 1, 1)
    rows_k, rows_v = k[:1, :, :LEN].repeat(B, 1, 1, 1), v[:1, :, :LEN].repeat(B, 1, 1, 1)
    k_row, v_row = k[:B, :, LEN:LEN + 1].contiguous(), v[:B, :, LEN:LEN + 1].contiguous()
    lens = torch.full((B,), LEN, dtype=torch.int32, device=dev)
    caches = {}
    perm = torch.randperm(2 * B * MAX_PAGES, generator=torch.Generator().manual_seed(5)).to(torch.int32).to(dev).view(2 * B, MAX_PAGES)
    private = PagedQuantizedKVCache.allocate(2 * B * MAX_PAGES, PAGE, B, MAX_PAGES, HKV, D, k.dtype, dev)
    private.block_table.copy_(perm[:B])
    private.seed(km, va)
    private.append(rows_k, rows_v, lens)
    shared = PagedQuantizedKVCache.allocate(2 * B * MAX_PAGES, PAGE, B, MAX_PAGES, HKV, D, k.dtype, dev)
    shared.block_table.copy_(perm[B:])
    shared.seed(km, va)
    shared.append(rows_k, rows_v, torch.tensor([LEN] + [0] * (B - 1), dtype=torch.int32, device=dev))
    shared.fork([0] * (B - 1), list(range(1, B)), perm[B + 1:, OWNED - 1].tolist())
    assert bool((shared.block_table[:, :OWNED - 1] == shared.block_table[0, :OWNED - 1]).all()) and shared.block_table[:, OWNED - 1].unique().numel() == B
    contig = QuantizedKVCache.allocate(B, HKV, MAX_PAGES * PAGE, D, k.dtype, dev)
    contig.seed(km, va)
    contig.append(rows_k, rows_v, lens)
    caches = {"shared": shared, "private": private, "contig": contig}
    fns, outs = {}, {}
    for name, c in caches.items():
        assert torch.equal(c.lens, lens)

        def reset(c=c):
            c.lens.copy_(lens)

        def set1(c=c):
            c.lens.copy_(lens + 1)

        def attn(c=c):
            return sageattn_kvcache(q, c, **KW)

        def step(c=c):
            c.append(k_row, v_row)
            return sageattn_kvcache(q, c, **KW)

        fns[f"{name}_attn"] = (set1, attn)
        fns[f"{name}_step"] = (reset, step)
        reset()
        outs[name] = step()
        assert torch.equal(attn(), outs[name])
    for name in caches:
        assert torch.equal(outs[name], outs["contig"]), f"{name}: the step must give the contiguous cache's bits"
    return fns


def time_interleaved(fns, rounds, reps):
    """us per call: {variant: [median of round 0, round 1, ...]}"""
    per_round = {n: [] for n in fns}
    for _ in range(rounds):
        for n, (setup, fn) in fns.items():
            for _ in range(3):
                setup()
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                setup()
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_fork_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kv_fork_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(19)
    nmax = max(max(FORKS), SHARERS)
    k, v = (torch.randn(nmax, HKV, LEN + 1, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(2))
    q = torch.randn(nmax, HQ, 1, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D 128, Hq 32 / Hkv 8, 8092 keys per "
                   "sequence in pages of 256 keys (31 whole pages and an open one of 156 keys); fork_N = PagedQuantizedKVCache.fork of N sequences in "
                   "one launch, refill_N = seed(slots=) + append of the 8092 raw rows into the N new slots; shared / private / contig: 32 sequences "
                   "of the same keys as 31 forks of one parent (whole pages shared), in pages of their own, in a contiguous QuantizedKVCache; "
                   "*_attn = sageattn_kvcache alone (Lq 1, bottom-right, pack_gqa), *_step = append(1 row) + sageattn_kvcache; spread = range of the "
                   "round medians / the figure; *_over_* = ratio of the figures of the same run; *_outside_contig_spread = the figure lies outside "
                   "the range of the contiguous variant's round medians",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "forks": [], "sharing": None}
    for n in FORKS:
        r = {"N": n}
        r.update(summary(time_interleaved(fork_variants(k[:, :, :LEN], v[:, :, :LEN], q, n), a.rounds, a.reps)))
        r["refill_over_fork"] = round(r[f"refill_{n}"]["us"] / r[f"fork_{n}"]["us"], 2)
        res["forks"].append(r)
        print(f"N {n:2d}: fork {r[f'fork_{n}']['us']:8.1f} us (spread {r[f'fork_{n}']['spread']:.3f})  seed + append of the raw rows {r[f'refill_{n}']['us']:9.1f} us "
              f"(spread {r[f'refill_{n}']['spread']:.3f})  x{r['refill_over_fork']:.1f}", flush=True)
        torch.cuda.empty_cache()
    per_round = time_interleaved(step_variants(k, v, q[:SHARERS]), a.rounds, a.reps)
    r = summary(per_round)
    for what in ("attn", "step"):
        base = per_round[f"contig_{what}"]
        r[f"shared_{what}_over_private"] = round(r[f"shared_{what}"]["us"] / r[f"private_{what}"]["us"], 4)
        for name in ("shared", "private"):
            r[f"{name}_{what}_over_contig"] = round(r[f"{name}_{what}"]["us"] / r[f"contig_{what}"]["us"], 4)
            r[f"{name}_{what}_outside_contig_spread"] = not (min(base) <= r[f"{name}_{what}"]["us"] <= max(base))
        print(f"{what}: shared {r[f'shared_{what}']['us']:7.1f} us  private {r[f'private_{what}']['us']:7.1f} us  contig {r[f'contig_{what}']['us']:7.1f} us "
              f"(spread {r[f'contig_{what}']['spread']:.3f})  shared / private x{r[f'shared_{what}_over_private']:.4f}", flush=True)
    res["sharing"] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
