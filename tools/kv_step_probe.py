#!/usr/bin/env python3
"""What the step call costs against the ragged call, the two-call split and the dense packed decode call (sageattention_amd.paged_kv_step,
DESIGN.md 3.22).

Shapes, steps and method are tools/kv_varlen_probe.py's: bf16, D 128, Hq 32 / Hkv 8, pages of 256 keys, contexts alternating 4096 / 8192 keys;
per round every variant is warmed, then timed call by call with device events; a figure is the median over the interleaved rounds of the
round's median, "spread" the range of the round medians relative to it.  Bits are checked before anything is timed.

Mixed steps -- N decode rows (one new token each) plus 4 prefill chunks of 512 rows in the last four slots, N = 28 and 124:
  step     sageattn_kvcache_step(q [total, Hq, D], cache, cu_seqlens_q, 512)       -- one call, two launches: packed decode groups, then chunks
  ragged   sageattn_kvcache_varlen(q, cache, cu_seqlens_q, 512)                    -- the parent's route: its kernels' listings are unchanged
  split    sageattn_kvcache(decode slots, pack_gqa=True) + sageattn_kvcache(chunk slots)   -- (b) of kv_varlen_probe: two calls on views of the cache
  step_spread / ragged_spread   the two calls with the same sequences in another slot order, the four chunks at slots 0, B/4, B/2, 3B/4 (kv_varlen_probe's
           ragged_spread): the chunk launch keeps the ragged launch's work order, which hands each XCD one contiguous run of (slot, head)
           pairs, so four adjacent chunk slots are one XCD's work -- the difference to `step` is what the chunk launch loses to slot order
Pure decode steps -- N rows, max_seqlen_q = 1, N = 28 and 124:
  step     sageattn_kvcache_step(q [N, Hq, D], cache, cu_seqlens_q, 1)              -- one launch
  ragged   sageattn_kvcache_varlen(q, cache, cu_seqlens_q, 1)
  dense    sageattn_kvcache(q [N, 1, Hq, D], cache, pack_gqa=True)                 -- the dense packed decode call
  step_idle_chunks   the step call on the same rows with max_seqlen_q = 512: its second launch of N * Hq * 4 workgroups runs, and every one
           of them leaves after the two prefix words -- minus `step`, what the chunk launch's early exits cost a mixed step of N + 4 slots
No ratio here is an acceptance bar.

    python tools/kv_step_probe.py [--rounds 5] [--reps 10] [--out profiles/kv_step_probe.json]
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

from kv_varlen_probe import CHUNK, CHUNKS, CONTEXTS, D, DISTINCT, HKV, HQ, MAX_PAGES, PAGE, _view, time_interleaved  # noqa: E402
from sageattention_amd.kv_cache import sageattn_kvcache  # noqa: E402
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache  # noqa: E402
from sageattention_amd.paged_kv_step import sageattn_kvcache_step  # noqa: E402
from sageattention_amd.paged_kv_varlen import sageattn_kvcache_varlen  # noqa: E402


def _filled(counts, seed, dev):
    """A cache of len(counts) sequences whose contexts (the step's rows included) alternate CONTEXTS, the packed queries and their prefix array."""
    B = len(counts)
    ctx = [CONTEXTS[b % 2] for b in range(B)]
    g = torch.Generator(device=dev).manual_seed(seed)
    k0, v0 = (torch.randn(DISTINCT, HKV, max(CONTEXTS), D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(2))
    k, v = k0.repeat(B // DISTINCT, 1, 1, 1), v0.repeat(B // DISTINCT, 1, 1, 1)
    c = PagedQuantizedKVCache.allocate(B * MAX_PAGES, PAGE, B, MAX_PAGES, HKV, D, torch.bfloat16, dev)
    c.block_table.copy_(torch.randperm(B * MAX_PAGES, generator=torch.Generator().manual_seed(seed)).to(torch.int32).to(dev).view(B, MAX_PAGES))
    c.seed(k.float().mean(dim=2).to(k.dtype), v.abs().float().amax(dim=2) * 2.0)
    c.append(k, v, torch.tensor(ctx, dtype=torch.int32, device=dev))
    cu = torch.tensor([sum(counts[:b]) for b in range(B + 1)], dtype=torch.int32, device=dev)
    q = torch.randn(sum(counts), HQ, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    return c, q, cu


def _nothing():
    pass


def mixed(nd, dev):
    counts = [1] * nd + [CHUNK] * CHUNKS
    c, q, cu = _filled(counts, 31 + nd, dev)
    q_dec, q_chk = q[:nd].unsqueeze(1).contiguous(), q[nd:].view(CHUNKS, CHUNK, HQ, D)
    dec, chk = _view(c, 0, nd), _view(c, nd, nd + CHUNKS)
    br = dict(tensor_layout="NHD", is_causal=True, causal_align="bottom_right")
    fns = {"step": lambda: sageattn_kvcache_step(q, c, cu, CHUNK),
           "ragged": lambda: sageattn_kvcache_varlen(q, c, cu, CHUNK),
           "split": lambda: (sageattn_kvcache(q_dec, dec, pack_gqa=True, **br), sageattn_kvcache(q_chk, chk, **br))}
    # the same sequences in another slot order (the per-sequence tensors gathered, the pool shared): the chunks B / 4 slots apart
    B = nd + CHUNKS
    order = list(range(nd))
    for j in range(CHUNKS):
        order.insert(j * (B // CHUNKS), nd + j)
    idx = torch.tensor(order, device=dev)
    spread = PagedQuantizedKVCache(c.num_pages, c.page_size, B, c.max_pages_per_seq, c.Hkv, c.D, c.dtype,
                                   (c.k_int8, c.k_scale, c.v_image) + tuple(t.index_select(0, idx) for t in (c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail,
                                                                                                           c.lens, c.block_table)))
    spread._seeded = True
    q_s = torch.cat([q[int(cu[i]):int(cu[i + 1])] for i in order])
    counts_s = [counts[i] for i in order]
    cu_s = torch.tensor([sum(counts_s[:b]) for b in range(B + 1)], dtype=torch.int32, device=dev)
    fns["step_spread"] = lambda: sageattn_kvcache_step(q_s, spread, cu_s, CHUNK)
    fns["ragged_spread"] = lambda: sageattn_kvcache_varlen(q_s, spread, cu_s, CHUNK)
    o, orag, (od, oc) = fns["step"](), fns["ragged"](), fns["split"]()
    os_, ors = fns["step_spread"](), fns["ragged_spread"]()
    assert torch.equal(os_.view(torch.int16), ors.view(torch.int16)), "step != ragged (spread)"
    assert all(torch.equal(os_[int(cu_s[i]):int(cu_s[i + 1])], o[int(cu[j]):int(cu[j + 1])]) for i, j in enumerate(order)), "slot order changed bits"
    assert torch.equal(o.view(torch.int16), orag.view(torch.int16)), "step != ragged"
    assert torch.equal(o[:nd], od[:, 0]) and torch.equal(o[nd:], oc.reshape(CHUNKS * CHUNK, HQ, D)), "step != the two calls"
    assert bool(torch.isfinite(o.float()).all())
    return {n: (_nothing, f) for n, f in fns.items()}, sum(counts)


def decode(nd, dev):
    c, q, cu = _filled([1] * nd, 77 + nd, dev)
    q_dense = q.unsqueeze(1).contiguous()
    br = dict(tensor_layout="NHD", is_causal=True, causal_align="bottom_right")
    fns = {"step": lambda: sageattn_kvcache_step(q, c, cu, 1),
           "ragged": lambda: sageattn_kvcache_varlen(q, c, cu, 1),
           "dense": lambda: sageattn_kvcache(q_dense, c, pack_gqa=True, **br),
           "step_idle_chunks": lambda: sageattn_kvcache_step(q, c, cu, CHUNK)}
    o, orag, od, oi = (fns[n]() for n in ("step", "ragged", "dense", "step_idle_chunks"))
    assert torch.equal(o.view(torch.int16), orag.view(torch.int16)) and torch.equal(o, od[:, 0]) and torch.equal(o.view(torch.int16), oi.view(torch.int16))
    assert bool(torch.isfinite(o.float()).all())
    return {n: (_nothing, f) for n, f in fns.items()}, nd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_step_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kv_step_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D 128, Hq 32 / Hkv 8, pages of 256 keys, contexts "
                   "alternating 4096 / 8192 keys.  mixed: N decode rows + 4 chunks of 512 rows; step = one sageattn_kvcache_step, ragged = one "
                   "sageattn_kvcache_varlen (the parent's kernels, listings unchanged), split = the decode rows through pack_gqa=True plus the chunks dense, two "
                   "calls on views of the cache, step_spread / ragged_spread = step / ragged with the chunks at slots 0, B/4, B/2, 3B/4 instead of the last four.  decode: N rows, max_seqlen_q 1; dense = sageattn_kvcache(pack_gqa=True) on q [N, 1, Hq, D]; step_idle_chunks = "
                   "the step call on the same rows with max_seqlen_q 512 (a second launch of N * Hq * 4 workgroups that all leave at once).  spread = range "
                   "of the round medians / the figure; x_over_y = ratio of the figures of the same run",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "mixed": [], "decode": []}
    for kind, build, pairs in (("mixed", mixed, (("step", "ragged"), ("step", "split"), ("ragged", "split"), ("step_spread", "ragged_spread"), ("step_spread", "split"), ("step_spread", "step"))),
                               ("decode", decode, (("step", "dense"), ("step", "ragged"), ("step_idle_chunks", "step")))):
        for nd in (28, 124):
            fns, total = build(nd, dev)
            per_round = time_interleaved(fns, a.rounds, a.reps)
            r = {"decode_rows": nd, "packed_rows": total}
            for n, xs in per_round.items():
                med = statistics.median(xs)
                r[n] = {"us": round(med, 1), "spread": round((max(xs) - min(xs)) / med, 4), "us_rounds": [round(x, 1) for x in xs]}
            for x, y in pairs:
                r[f"{x}_over_{y}"] = round(r[x]["us"] / r[y]["us"], 4)
            res[kind].append(r)
            print(f"{kind} N {nd:3d}: " + "  ".join(f"{n} {r[n]['us']:8.1f} us (+-{100 * r[n]['spread']:.1f}%)" for n in fns) + "  " +
                  "  ".join(f"{x}/{y} x{r[f'{x}_over_{y}']:.3f}" for x, y in pairs), flush=True)
            del fns
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
