#!/usr/bin/env python3
"""What the exact split (num_splits=) costs and buys on the PAGED quantised KV cache (sageattention_amd.paged_kv_split): the paged
unsplit call, the paged split at S = 8 / 16 / 32 and "auto", and the contiguous cache's split at the same S, interleaved in one process.

Shapes (the packed rows of tools/num_splits_probe.py): bf16, D 128, Hq 32 / Hkv 8, Lq 1, pack_gqa=True, causal with
causal_align="bottom_right" and the lengths drawn (seeded) from [Lk / 2, Lk]; B 1 / 4 / 8; Lk 8192 / 32768 / 65536 keys of capacity.  Pages of
64 and of 256 keys; the block table is a random permutation over a pool of twice the pages the batch needs.

"contig_unsplit" / "contig_s8" ...    sageattn_kvcache(q, contiguous cache, num_splits=...)
"pagedN_unsplit" / "pagedN_s8" ...    sageattn_kvcache_split(q, paged cache with pages of N keys, ...): the attention launches behind the same
                                      Python layer (unsplit: one launch; a split: pass 1 + pass 2 + merge)
All three caches are filled from one prompt with the same statistics, and before anything is timed every paged output is compared with the
contiguous cache's at the same S bit for bit.

Per round every variant is warmed, then timed call by call with device events; the figure of a variant is the median over the rounds of the
round's median, "spread" the range of the round medians relative to it.  What is compared, next to the contiguous call's own spread:
  pagedN_sS_over_contig    paged split / contiguous split at the same S: the cost of paging inside the split
  pagedN_sS_over_unsplit   paged split / paged unsplit: what the feature buys
  pagedN_auto_slower       the auto plan chose a split that is slower than the unsplit paged call by more than the larger of the two spreads

    python tools/paged_split_probe.py [--rounds 5] [--reps 8] [--out profiles/paged_split_probe.json] [--lk 8192,32768,65536] [--batches 1,4,8]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sageattention_amd import core  # noqa: E402
from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache  # noqa: E402
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache  # noqa: E402
from sageattention_amd.paged_kv_split import sageattn_kvcache_split  # noqa: E402

HQ, HKV, D, LQ = 32, 8, 128, 1
SPLITS = (8, 16, 32)
PAGE_SIZES = (64, 256)
KW = dict(is_causal=True, causal_align="bottom_right", pack_gqa=True)


def variants(q, k, v, lens, Lk):
    """{name: callable} on one batch, and the auto plan's S"""
    B = q.shape[0]
    caches = {"contig": QuantizedKVCache.from_prefill(k, v, Lk, kv_lens=lens)}
    for ps in PAGE_SIZES:
        need = B * (Lk // ps)
        perm = torch.randperm(2 * need, generator=torch.Generator().manual_seed(ps))[:need]
        caches[f"paged{ps}"] = PagedQuantizedKVCache.from_prefill(k, v, perm.view(B, Lk // ps).to(q.device), 2 * need, ps, kv_lens=lens)
    auto = core._num_splits_plan(B, HQ, HKV, LQ, Lk, True)
    fns = {}
    for name, c in caches.items():
        for tag, s in [("unsplit", None)] + [(f"s{s}", s) for s in SPLITS] + [("auto", "auto")]:
            if name == "contig":
                fns[f"{name}_{tag}"] = lambda c=c, s=s: sageattn_kvcache(q, c, num_splits=s, **KW)
            else:
                fns[f"{name}_{tag}"] = lambda c=c, s=s: sageattn_kvcache_split(q, c, s, **KW)
    outs = {n: fn() for n, fn in fns.items()}
    torch.cuda.synchronize()
    for n, o in outs.items():
        ref = outs["contig_" + n.split("_", 1)[1]]
        assert torch.equal(o, ref), f"{n}: a paged call must give the contiguous cache's bits at the same S"
    return fns, auto


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


def summary(per_round, auto):
    out = {}
    for n, xs in per_round.items():
        med = statistics.median(xs)
        out[n] = {"us": round(med, 1), "spread": round((max(xs) - min(xs)) / med, 4), "us_rounds": [round(x, 1) for x in xs]}
    for ps in PAGE_SIZES:
        un = out[f"paged{ps}_unsplit"]
        out[f"paged{ps}_unsplit_over_contig"] = round(un["us"] / out["contig_unsplit"]["us"], 4)
        for tag in [f"s{s}" for s in SPLITS] + ["auto"]:
            me, contig = out[f"paged{ps}_{tag}"], out[f"contig_{tag}"]
            out[f"paged{ps}_{tag}_over_contig"] = round(me["us"] / contig["us"], 4)
            out[f"paged{ps}_{tag}_over_unsplit"] = round(me["us"] / un["us"], 4)
        a = out[f"paged{ps}_auto"]
        out[f"paged{ps}_auto_slower"] = bool(auto) and a["us"] > un["us"] * (1.0 + max(a["spread"], un["spread"], out["contig_auto"]["spread"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--lk", default="8192,32768,65536")
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged_split_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "paged_split_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    lks, batches = [int(x) for x in a.lk.split(",")], [int(x) for x in a.batches.split(",")]
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D 128, Hq 32 / Hkv 8, Lq 1, pack_gqa=True, "
                   "causal_align='bottom_right', lengths drawn from [Lk / 2, Lk]; contig = QuantizedKVCache with sageattn_kvcache(num_splits=), pagedN = "
                   "PagedQuantizedKVCache with pages of N keys behind a random permutation over a pool of twice the need, with sageattn_kvcache_split; "
                   "spread = range of the round medians / the figure; *_over_contig = paged / contiguous at the same S; *_over_unsplit = paged split / "
                   "paged unsplit; *_auto_slower = the auto plan's split is slower than the unsplit paged call by more than the larger spread",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "shapes": []}
    for Lk in lks:
        g = torch.Generator(device=dev).manual_seed(15 + Lk)
        bmax = max(batches)
        k_all, v_all = (torch.randn(bmax, HKV, Lk, D, generator=g, device=dev, dtype=torch.bfloat16) for _ in range(2))
        q_all = torch.randn(bmax, HQ, LQ, D, generator=g, device=dev, dtype=torch.bfloat16)
        lens_all = torch.randint(Lk // 2, Lk + 1, (bmax,), generator=torch.Generator().manual_seed(15)).to(torch.int32)
        for B in batches:
            q, k, v = q_all[:B], k_all[:B], v_all[:B]
            lens = lens_all[:B].to(dev)
            fns, auto = variants(q, k, v, lens, Lk)
            r = {"B": B, "Lq": LQ, "Lk": Lk, "workgroups_unsplit": B * HKV, "auto_S": auto, "lens_min_max": [int(lens.min()), int(lens.max())]}
            r.update(summary(time_interleaved(fns, a.rounds, a.reps), auto))
            res["shapes"].append(r)
            for ps in PAGE_SIZES:
                print(f"Lk {Lk:6d} B {B} page {ps:3d}: unsplit {r[f'paged{ps}_unsplit']['us']:8.1f} us (x{r[f'paged{ps}_unsplit_over_contig']:.3f} of contig)  "
                      + "  ".join(f"{t} {r[f'paged{ps}_{t}']['us']:7.1f} us (x{r[f'paged{ps}_{t}_over_contig']:.3f} of contig, x{r[f'paged{ps}_{t}_over_unsplit']:.3f} of unsplit)"
                                  for t in [f"s{s}" for s in SPLITS] + ["auto"])
                      + f"  auto S={auto} slower={r[f'paged{ps}_auto_slower']}  contig spreads unsplit {r['contig_unsplit']['spread']:.3f} s8 {r['contig_s8']['spread']:.3f}", flush=True)
            res["auto_slower_anywhere"] = any(r[f"paged{ps}_auto_slower"] for r in res["shapes"] for ps in PAGE_SIZES)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:                     # (after every shape: a run cut short leaves what it measured)
                json.dump(res, f, indent=1)
            del fns
            torch.cuda.empty_cache()
        del k_all, v_all, q_all
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
