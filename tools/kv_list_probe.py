#!/usr/bin/env python3
"""What the listed step call costs against the step call, the ragged call and the caller's two calls (sageattention_amd.paged_kv_list,
DESIGN.md 3.23).

Shapes, steps and method are tools/kv_step_probe.py's: bf16, D 128, Hq 32 / Hkv 8, pages of 256 keys, contexts alternating 4096 / 8192 keys;
per round every variant is warmed, then timed call by call with device events; a figure is the median over the interleaved rounds of the
round's median, "spread" the range of the round medians relative to it.  Bits are checked before anything is timed.

Mixed steps -- N decode rows plus 4 prefill chunks of 512 rows, N = 28 and 124, the chunks in the last four slots and (`*_spread`) at slots
0, B/4, B/2, 3B/4:
  listed   sageattn_kvcache_step_listed(q, cache, cu_seqlens_q, 512)     -- three launches: plan, decode list, chunk list
  step     sageattn_kvcache_step(q, cache, cu_seqlens_q, 512)            -- the parent's call: its kernels' listings are unchanged
  ragged   sageattn_kvcache_varlen(q, cache, cu_seqlens_q, 512)
  split    sageattn_kvcache(decode slots, pack_gqa=True) + sageattn_kvcache(chunk slots)     -- (b): the caller's two calls
  plan     sage_kvlist_plan alone on the step's words
Pure decode steps -- N rows, max_seqlen_q = 1, N = 28 and 124: listed, step, ragged, plan.
One pure decode step of 128 rows whose contexts differ by 16x in adjacent slots -- the first sixteen slots hold 8192 keys, the others 512, so
the step call's contiguous runs hand XCD 0 every long context: listed, step, ragged, plan.
No ratio here is an acceptance bar.

    python tools/kv_list_probe.py [--rounds 5] [--reps 10] [--out profiles/kv_list_probe.json]
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
from kv_varlen_probe import CHUNK, CHUNKS, CONTEXTS, D, DISTINCT, HKV, HQ, MAX_PAGES, PAGE, _view, time_interleaved  # noqa: E402
from sageattention_amd import _cabi_kvlist  # noqa: E402
from sageattention_amd.kv_cache import sageattn_kvcache  # noqa: E402
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache  # noqa: E402
from sageattention_amd.paged_kv_list import sageattn_kvcache_step_listed  # noqa: E402
from sageattention_amd.paged_kv_step import sageattn_kvcache_step  # noqa: E402
from sageattention_amd.paged_kv_varlen import sageattn_kvcache_varlen  # noqa: E402
from sageattention_amd.quant import _p, _stream  # noqa: E402


def _filled(counts, ctx, seed, dev):
    """A cache of len(counts) sequences with contexts ``ctx`` (the step's rows included), the packed queries and their prefix array."""
    B = len(counts)
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


def _plan_alone(c, q, cu, max_q):
    """The plan launch by itself, on the words the listed call hands it (bottom-right offsets)."""
    lib = _cabi_kvlist.load()
    B, total = c.B, q.shape[0]
    start = (c.lens.clamp(0, c.capacity).to(torch.int64) - (cu[1:] - cu[:-1]).to(torch.int64)).to(torch.int32)
    nbytes = lib.sage_kvlist_ws_bytes(B, total, max_q)
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=q.device)

    def run():
        rc = lib.sage_kvlist_plan(_p(cu), _p(c.lens), _p(start), B, total, max_q, c.capacity, 0, HQ, HKV, D, _p(ws), nbytes, _stream(q))
        assert rc == 0, lib.sage_last_error()
    return run


def _same(a, b, what):
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), what


def mixed(nd, dev):
    counts = [1] * nd + [CHUNK] * CHUNKS
    B = nd + CHUNKS
    c, q, cu = _filled(counts, [CONTEXTS[b % 2] for b in range(B)], 31 + nd, dev)
    q_dec, q_chk = q[:nd].unsqueeze(1).contiguous(), q[nd:].view(CHUNKS, CHUNK, HQ, D)
    dec, chk = _view(c, 0, nd), _view(c, nd, nd + CHUNKS)
    br = dict(tensor_layout="NHD", is_causal=True, causal_align="bottom_right")
    fns = {"listed": lambda: sageattn_kvcache_step_listed(q, c, cu, CHUNK),
           "step": lambda: sageattn_kvcache_step(q, c, cu, CHUNK),
           "ragged": lambda: sageattn_kvcache_varlen(q, c, cu, CHUNK),
           "split": lambda: (sageattn_kvcache(q_dec, dec, pack_gqa=True, **br), sageattn_kvcache(q_chk, chk, **br)),
           "plan": _plan_alone(c, q, cu, CHUNK)}
    # the same sequences in another slot order (the per-sequence tensors gathered, the pool shared): the chunks B / 4 slots apart
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
    fns["listed_spread"] = lambda: sageattn_kvcache_step_listed(q_s, spread, cu_s, CHUNK)
    fns["step_spread"] = lambda: sageattn_kvcache_step(q_s, spread, cu_s, CHUNK)
    fns["ragged_spread"] = lambda: sageattn_kvcache_varlen(q_s, spread, cu_s, CHUNK)
    o, ost, orag, (od, oc) = fns["listed"](), fns["step"](), fns["ragged"](), fns["split"]()
    _same(o, ost, "listed != step")
    _same(o, orag, "listed != ragged")
    assert torch.equal(o[:nd], od[:, 0]) and torch.equal(o[nd:], oc.reshape(CHUNKS * CHUNK, HQ, D)), "listed != the two calls"
    ols = fns["listed_spread"]()
    _same(ols, fns["step_spread"](), "listed != step (spread)")
    _same(ols, fns["ragged_spread"](), "listed != ragged (spread)")
    assert all(torch.equal(ols[int(cu_s[i]):int(cu_s[i + 1])], o[int(cu[j]):int(cu[j + 1])]) for i, j in enumerate(order)), "slot order changed bits"
    assert bool(torch.isfinite(o.float()).all())
    fns["plan"]()
    return {n: (_nothing, f) for n, f in fns.items()}, sum(counts)


def decode(nd, dev, ctx=None):
    c, q, cu = _filled([1] * nd, ctx or [CONTEXTS[b % 2] for b in range(nd)], 77 + nd + (1 if ctx else 0), dev)
    fns = {"listed": lambda: sageattn_kvcache_step_listed(q, c, cu, 1),
           "step": lambda: sageattn_kvcache_step(q, c, cu, 1),
           "ragged": lambda: sageattn_kvcache_varlen(q, c, cu, 1),
           "plan": _plan_alone(c, q, cu, 1)}
    o = fns["listed"]()
    _same(o, fns["step"](), "listed != step")
    _same(o, fns["ragged"](), "listed != ragged")
    assert bool(torch.isfinite(o.float()).all())
    fns["plan"]()
    return {n: (_nothing, f) for n, f in fns.items()}, nd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_list_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kv_list_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D 128, Hq 32 / Hkv 8, pages of 256 keys, contexts "
                   "alternating 4096 / 8192 keys.  mixed: N decode rows + 4 chunks of 512 rows; listed = one sageattn_kvcache_step_listed (plan + two launches over "
                   "device-built lists), step = one sageattn_kvcache_step (the parent's kernels, listings unchanged), ragged = one sageattn_kvcache_varlen, split = "
                   "the decode rows through pack_gqa=True plus the chunks dense, two calls on views of the cache, plan = sage_kvlist_plan alone; *_spread = the "
                   "same sequences with the chunks at slots 0, B/4, B/2, 3B/4 instead of the last four.  decode: N rows, max_seqlen_q 1.  decode_skewed: 128 rows, "
                   "the first sixteen slots hold 8192 keys and the others 512.  spread = range of the round medians / the figure; x_over_y = ratio of the figures "
                   "of the same run",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "mixed": [], "decode": [], "decode_skewed": []}
    mixed_pairs = (("listed", "step"), ("listed", "ragged"), ("listed", "split"), ("listed_spread", "step_spread"), ("listed_spread", "ragged_spread"),
                   ("listed_spread", "split"), ("listed_spread", "listed"), ("plan", "listed"))
    decode_pairs = (("listed", "step"), ("listed", "ragged"), ("plan", "listed"))
    skewed = [max(CONTEXTS)] * 16 + [max(CONTEXTS) // 16] * 112
    for kind, build, pairs, sizes in (("mixed", mixed, mixed_pairs, (28, 124)), ("decode", decode, decode_pairs, (28, 124)),
                                      ("decode_skewed", lambda nd, dev: decode(nd, dev, skewed), decode_pairs, (128,))):
        for nd in sizes:
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
