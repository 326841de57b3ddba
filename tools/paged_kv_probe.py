#!/usr/bin/env python3
"""What a block table costs one decode step of the quantised KV cache (sageattention_amd.paged_kv_cache): the contiguous
cache's attention call and whole step (append one row + attend) against the paged cache's, interleaved in one process.

Shapes (those of tools/kv_cache_probe.py): bf16, D 128, Hq 32 / Hkv 8, 8192 keys of capacity, Lq 1, causal with
causal_align="bottom_right", pack_gqa=True; B 4, 32 and 128; the lengths before the step drawn (seeded) from [Lk / 2, Lk - 1].  Pages of 64
and of 256 keys; the block table is a random permutation over a pool of twice the pages the batch needs.

"contig_attn" / "paged64_attn" / "paged256_attn"   sageattn_kvcache(q, cache, ...) alone: the attention launch behind the same Python layer
"contig_step" / "paged64_step" / "paged256_step"   cache.append(one row) + sageattn_kvcache(q, cache, ...)
Before every timed step the cache's lengths are put back to the drawn ones, outside the timed interval.  All three caches are seeded with the
same statistics, and before anything is timed the paged outputs are compared with the contiguous cache's bit for bit.

Per round every variant is warmed, then timed call by call with device events; the figure of a variant is the median over the rounds of the
round's median, "spread" the range of the round medians relative to it.  The ratios are against the contiguous figure of the same run, and
"outside_contig_spread" says whether the paged figure lies outside the range of the contiguous variant's own round medians.

    python tools/paged_kv_probe.py [--rounds 5] [--reps 10] [--out profiles/paged_kv_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sageattention_amd import quant  # noqa: E402
from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache  # noqa: E402
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache  # noqa: E402

HQ, HKV, LK, D = 32, 8, 8192, 128
BATCHES, LQ = (4, 32, 128), 1
PAGE_SIZES = (64, 256)
KW = dict(is_causal=True, causal_align="bottom_right", pack_gqa=True)


def variants(q, k, v, lens):
    """{name: (untimed setup, timed call)} on one batch; ``k`` / ``v`` hold row ``lens[b]``, the row the step adds."""
    B = q.shape[0]
    lens1 = lens + 1
    idx = lens.long().view(B, 1, 1, 1).expand(B, HKV, 1, D)
    k_row, v_row = k.gather(2, idx).contiguous(), v.gather(2, idx).contiguous()
    valid = (torch.arange(LK, device=q.device)[None, :] < lens1[:, None]).view(B, 1, LK, 1)
    km, va = quant.channel_mean_kvlens(k, lens1), torch.where(valid, v.abs().float(), 0.0).amax(dim=2)
    caches = {"contig": QuantizedKVCache.allocate(B, HKV, LK, D, q.dtype, q.device)}
    for ps in PAGE_SIZES:
        need = B * (LK // ps)
        c = PagedQuantizedKVCache.allocate(2 * need, ps, B, LK // ps, HKV, D, q.dtype, q.device)
        perm = torch.randperm(2 * need, generator=torch.Generator().manual_seed(ps))[:need]
        c.block_table.copy_(perm.view(B, LK // ps).to(torch.int32))
        caches[f"paged{ps}"] = c
    fns = {}
    for name, c in caches.items():
        c.seed(km, va)
        c.append(k, v, lens)

        def reset(c=c):
            c.lens.copy_(lens)

        def set1(c=c):
            c.lens.copy_(lens1)

        def attn(c=c):
            return sageattn_kvcache(q, c, **KW)

        def step(c=c):
            c.append(k_row, v_row)
            return sageattn_kvcache(q, c, **KW)

        fns[f"{name}_attn"] = (set1, attn)
        fns[f"{name}_step"] = (reset, step)
    outs = {}
    for name in caches:
        fns[f"{name}_step"][0]()
        outs[name] = fns[f"{name}_step"][1]()
        assert torch.equal(caches[name].lens, lens1)
    for name in caches:
        assert torch.equal(outs[name], outs["contig"]), f"{name}: the paged step must give the contiguous cache's bits"
        assert torch.equal(fns[f"{name}_attn"][1](), outs["contig"])
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
    for what in ("attn", "step"):
        base = per_round[f"contig_{what}"]
        for ps in PAGE_SIZES:
            us = out[f"paged{ps}_{what}"]["us"]
            out[f"paged{ps}_{what}_over_contig"] = round(us / out[f"contig_{what}"]["us"], 4)
            out[f"paged{ps}_{what}_outside_contig_spread"] = not (min(base) <= us <= max(base))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged_kv_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "paged_kv_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(16)
    bmax = max(BATCHES)
    k_all, v_all = (torch.randn(bmax, HKV, LK, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(2))
    q_all = torch.randn(bmax, HQ, LQ, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    lens_all = torch.randint(LK // 2, LK, (bmax,), generator=torch.Generator().manual_seed(16)).to(torch.int32)
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D 128, Hq 32 / Hkv 8, 8192 keys of "
                   "capacity, Lq 1, causal_align='bottom_right', pack_gqa=True, lengths drawn from [Lk / 2, Lk - 1] plus the step's row; *_attn = "
                   "sageattn_kvcache alone, *_step = append(1 row) + sageattn_kvcache; contig = QuantizedKVCache, pagedN = PagedQuantizedKVCache with "
                   "pages of N keys behind a random permutation over a pool of twice the need; spread = range of the round medians / the figure; "
                   "*_over_contig = ratio to the contiguous figure of the same run; *_outside_contig_spread = the paged figure lies outside the "
                   "range of the contiguous variant's round medians",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "shapes": []}
    for B in BATCHES:
        q, k, v = q_all[:B], k_all[:B], v_all[:B]
        lens = lens_all[:B].to(dev)
        r = {"B": B, "Lq": LQ, "lens_min_max": [int(lens.min()), int(lens.max())]}
        r.update(summary(time_interleaved(variants(q, k, v, lens), a.rounds, a.reps)))
        res["shapes"].append(r)
        print(f"B {B:3d} attn: contig {r['contig_attn']['us']:7.1f} us (spread {r['contig_attn']['spread']:.3f})  "
              + "  ".join(f"paged{ps} {r[f'paged{ps}_attn']['us']:7.1f} us x{r[f'paged{ps}_attn_over_contig']:.4f}" for ps in PAGE_SIZES)
              + f" | step: contig {r['contig_step']['us']:7.1f} us (spread {r['contig_step']['spread']:.3f})  "
              + "  ".join(f"paged{ps} {r[f'paged{ps}_step']['us']:7.1f} us x{r[f'paged{ps}_step_over_contig']:.4f}" for ps in PAGE_SIZES), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
