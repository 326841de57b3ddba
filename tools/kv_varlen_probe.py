#!/usr/bin/env python3
"""What one packed call costs against the two things a caller can do without it (sageattention_amd.paged_kv_varlen).

Shape: bf16, D 128, Hq 32 / Hkv 8, pages of 256 keys, contexts (after the step's append) alternating 4096 / 8192 keys.  A mixed step of a
continuous-batching engine: N decode rows (slots 0 .. N - 1, one new token each) plus 4 prefill chunks of 512 rows (the last four slots), for
N = 28 and N = 124 -- 32 and 128 sequences, 2076 and 2172 packed rows.

Attention, bottom-right aligned, all three bit-equal on every row a sequence owns (checked before anything is timed):
  ragged   sageattn_kvcache_varlen(q [total, Hq, D], cache, cu_seqlens_q, 512)                            -- one call
  ragged_spread   the same call with the same sequences in another slot order: the four chunks at slots 0, B/4, B/2, 3B/4 instead of the last
           four.  The dense work order hands each XCD one contiguous run of (slot, head) pairs, so four adjacent chunk slots are one XCD's
           work; spread, they are four XCDs'.  What the difference says about a work list across sequences is DESIGN.md 3.21's to draw.
  padded   sageattn_kvcache(q [B, 512, Hq, D], cache, is_causal, q_start = lens - Lq_b)                    -- (a) every sequence padded to Lq 512
  split    sageattn_kvcache(q [N, 1, Hq, D], decode slots, pack_gqa=True) + sageattn_kvcache(q [4, 512, Hq, D], chunk slots)   -- (b) two calls, each
           on a view of the cache that holds its slots (the pool is shared, the per-sequence tensors are sliced)
The padded call's copies of the rows into and out of the padded tensors are NOT timed (they favour the packed call further); neither is the
forming of cu_seqlens.  Decode rows in the ragged call run one workgroup per query head -- the split's packed GQA groups run four heads per
workgroup over one K / V stream: what that costs the ragged call is the figure ragged_over_split.

Append of the step's new rows:
  append_ragged   append_varlen(cache, k_new [total, Hkv, D], v_new, cu_seqlens, 512)
  append_padded   cache.append(k_new [B, Hkv, 512, D], v_new, new_lens)
Before every timed append the lengths are put back, outside the timed interval.

Per round every variant is warmed, then timed call by call with device events; the figure of a variant is the median over the rounds of the
round's median, "spread" the range of the round medians relative to it.  No ratio here is an acceptance bar.

    python tools/kv_varlen_probe.py [--rounds 5] [--reps 10] [--out profiles/kv_varlen_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sageattention_amd.kv_cache import sageattn_kvcache  # noqa: E402
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache  # noqa: E402
from sageattention_amd.paged_kv_varlen import append_varlen, sageattn_kvcache_varlen  # noqa: E402

HQ, HKV, D, PAGE = 32, 8, 128, 256
CONTEXTS = (4096, 8192)
CHUNKS, CHUNK = 4, 512
MAX_PAGES = max(CONTEXTS) // PAGE + 1
DISTINCT = 4                                   # sequences with content of their own; the others repeat them (what is timed does not depend on it)


def _view(c, lo, hi):
    """The slots lo .. hi - 1 of ``c`` as a cache of their own over the same pool: what a caller that batches by kind holds."""
    sub = PagedQuantizedKVCache(c.num_pages, c.page_size, hi - lo, c.max_pages_per_seq, c.Hkv, c.D, c.dtype,
                                (c.k_int8, c.k_scale, c.v_image, c.v_scale[lo:hi], c.v_amax[lo:hi], c.k_mean[lo:hi], c.k_tail[lo:hi], c.v_tail[lo:hi],
                                 c.lens[lo:hi], c.block_table[lo:hi]))
    sub._seeded = True
    return sub


def variants(nd, dev):
    """{name: (untimed setup, timed call)} of the step with ``nd`` decode rows"""
    B = nd + CHUNKS
    counts = [1] * nd + [CHUNK] * CHUNKS
    ctx = [CONTEXTS[b % 2] for b in range(B)]
    total = sum(counts)
    g = torch.Generator(device=dev).manual_seed(31 + nd)
    k0, v0 = (torch.randn(DISTINCT, HKV, max(CONTEXTS), D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(2))
    k, v = k0.repeat(B // DISTINCT, 1, 1, 1), v0.repeat(B // DISTINCT, 1, 1, 1)
    c = PagedQuantizedKVCache.allocate(B * MAX_PAGES, PAGE, B, MAX_PAGES, HKV, D, torch.bfloat16, dev)
    c.block_table.copy_(torch.randperm(B * MAX_PAGES, generator=torch.Generator().manual_seed(nd)).to(torch.int32).to(dev).view(B, MAX_PAGES))
    c.seed(k.float().mean(dim=2).to(k.dtype), v.abs().float().amax(dim=2) * 2.0)
    after = torch.tensor(ctx, dtype=torch.int32, device=dev)
    before = after - torch.tensor(counts, dtype=torch.int32, device=dev)
    c.append(k, v, before)                     # the context in front of the step
    cu = torch.tensor([sum(counts[:b]) for b in range(B + 1)], dtype=torch.int32, device=dev)
    # the step's new rows and queries, packed and padded
    k_new, v_new = (torch.empty(total, HKV, D, dtype=torch.bfloat16, device=dev) for _ in range(2))
    k_pad, v_pad = (torch.zeros(B, HKV, CHUNK, D, dtype=torch.bfloat16, device=dev) for _ in range(2))
    q = torch.randn(total, HQ, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    q_pad = torch.zeros(B, CHUNK, HQ, D, dtype=torch.bfloat16, device=dev)
    for b in range(B):
        lo, n = int(cu[b]), counts[b]
        k_new[lo:lo + n], v_new[lo:lo + n] = k[b, :, ctx[b] - n:ctx[b]].transpose(0, 1), v[b, :, ctx[b] - n:ctx[b]].transpose(0, 1)
        k_pad[b, :, :n], v_pad[b, :, :n] = k[b, :, ctx[b] - n:ctx[b]], v[b, :, ctx[b] - n:ctx[b]]
        q_pad[b, :n] = q[lo:lo + n]
    del k, v, k0, v0
    new_lens = torch.tensor(counts, dtype=torch.int32, device=dev)
    q_dec, q_chk = q[:nd].unsqueeze(1).contiguous(), q[nd:].view(CHUNKS, CHUNK, HQ, D)
    dec, chk = _view(c, 0, nd), _view(c, nd, B)
    br = dict(tensor_layout="NHD", is_causal=True, causal_align="bottom_right")

    def nothing():
        pass

    def rewind():
        c.lens.copy_(before)

    def ragged():
        return sageattn_kvcache_varlen(q, c, cu, CHUNK)

    # the same sequences in another slot order (the per-sequence tensors gathered, the pool shared): the chunks B/4 slots apart
    order = list(range(nd))
    for j in range(CHUNKS):
        order.insert(j * (B // CHUNKS), nd + j)
    idx = torch.tensor(order, device=dev)
    spread = PagedQuantizedKVCache(c.num_pages, c.page_size, B, c.max_pages_per_seq, c.Hkv, c.D, c.dtype,
                                   (c.k_int8, c.k_scale, c.v_image) + tuple(t.index_select(0, idx) for t in (c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail))
                                   + (after.index_select(0, idx), c.block_table.index_select(0, idx)))
    spread._seeded = True
    q_spread = torch.cat([q[int(cu[s]):int(cu[s + 1])] for s in order])
    counts_spread = [counts[s] for s in order]
    cu_spread = torch.tensor([sum(counts_spread[:b]) for b in range(B + 1)], dtype=torch.int32, device=dev)

    def ragged_spread():
        return sageattn_kvcache_varlen(q_spread, spread, cu_spread, CHUNK)

    def padded():
        return sageattn_kvcache(q_pad, c, tensor_layout="NHD", is_causal=True, q_start=before)

    def split():
        return sageattn_kvcache(q_dec, dec, pack_gqa=True, **br), sageattn_kvcache(q_chk, chk, **br)

    def append_ragged():
        append_varlen(c, k_new, v_new, cu, CHUNK)

    def append_padded():
        c.append(k_pad, v_pad, new_lens)

    # bits before timing: both appends give one cache, all three calls one output on every owned row
    rewind(); append_padded(); torch.cuda.synchronize()
    pool = [t.clone() for t in (c.k_int8, c.k_scale, c.v_image, c.k_tail, c.v_tail, c.lens)]
    rewind(); append_ragged(); torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b_.view(torch.uint8)) for a, b_ in zip(pool, (c.k_int8, c.k_scale, c.v_image, c.k_tail, c.v_tail, c.lens)))
    assert torch.equal(c.lens, after)
    del pool
    o, (od, oc), op = ragged(), split(), padded()
    assert torch.equal(o[:nd], od[:, 0]) and torch.equal(o[nd:], oc.reshape(CHUNKS * CHUNK, HQ, D)), "ragged != the two calls"
    assert all(torch.equal(o[int(cu[b]):int(cu[b + 1])], op[b, :counts[b]]) for b in range(B)), "ragged != the padded call"
    assert bool(torch.isfinite(o.float()).all())
    os_ = ragged_spread()
    assert all(torch.equal(os_[int(cu_spread[i]):int(cu_spread[i + 1])], o[int(cu[s]):int(cu[s + 1])]) for i, s in enumerate(order)), "slot order changed bits"
    return ({"ragged": (nothing, ragged), "ragged_spread": (nothing, ragged_spread), "padded": (nothing, padded), "split": (nothing, split),
             "append_ragged": (rewind, append_ragged), "append_padded": (rewind, append_padded)}, after, total)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_varlen_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kv_varlen_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D 128, Hq 32 / Hkv 8, pages of 256 keys, "
                   "contexts alternating 4096 / 8192 keys; a step of N decode rows + 4 chunks of 512 rows; ragged = one sageattn_kvcache_varlen (the chunks in the "
                   "last four slots), ragged_spread = the same call with the chunks at slots 0, B/4, B/2, 3B/4, padded = "
                   "sageattn_kvcache on q padded to Lq 512 with q_start (copies not timed), split = the decode rows through pack_gqa=True plus the chunks "
                   "dense, two calls on views of the cache; append_ragged = append_varlen of the packed rows, append_padded = append of rows padded to "
                   "T 512 with new_lens; spread = range of the round medians / the figure; x_over_y = ratio of the figures of the same run",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "steps": []}
    for nd in (28, 124):
        fns, after, total = variants(nd, dev)
        per_round = time_interleaved(fns, a.rounds, a.reps)
        r = {"decode_rows": nd, "chunks": CHUNKS, "chunk_rows": CHUNK, "sequences": nd + CHUNKS, "packed_rows": total}
        for n, xs in per_round.items():
            med = statistics.median(xs)
            r[n] = {"us": round(med, 1), "spread": round((max(xs) - min(xs)) / med, 4), "us_rounds": [round(x, 1) for x in xs]}
        for x, y in (("ragged", "padded"), ("ragged", "split"), ("ragged_spread", "ragged"), ("ragged_spread", "split"), ("append_ragged", "append_padded")):
            r[f"{x}_over_{y}"] = round(r[x]["us"] / r[y]["us"], 4)
        res["steps"].append(r)
        print(f"N {nd:3d}: ragged {r['ragged']['us']:8.1f} us  spread {r['ragged_spread']['us']:8.1f} us  padded {r['padded']['us']:8.1f} us (x{r['ragged_over_padded']:.3f})  split {r['split']['us']:8.1f} us "
              f"(x{r['ragged_over_split']:.3f})  append ragged {r['append_ragged']['us']:7.1f} us  padded {r['append_padded']['us']:7.1f} us "
              f"(x{r['append_ragged_over_append_padded']:.3f})", flush=True)
        del fns
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
