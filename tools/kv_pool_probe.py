#!/usr/bin/env python3
"""What the page pool's launches cost next to the calls they stand in front of (sageattention_amd.paged_kv_pool).

Shapes of the README's KV-cache rows: bf16, D 128, Hq 32 / Hkv 8, pages of 256 keys, contexts alternating 4096 / 8192 keys, B 4 / 32 / 128.
Method of tools/kv_step_probe.py: per round every variant is warmed, then timed call by call with device events; a figure is the median over
the interleaved rounds of the round's median, "spread" the range of the round medians relative to it.  What a variant changes (lengths, table,
workspace) is put back from a snapshot in front of every call, outside the timed interval.  No ratio here is an acceptance bar.

Per B, one decode step (one new row per sequence):
  reserve_idle     pool.reserve(new_lens, T=1) when no sequence stands on a page boundary: nothing is popped
  reserve_pop      the same launch when EVERY sequence stands on a page boundary: B pages popped
  pool_append      pool.append(k_new, v_new): reserve + the append's two launches, the table kept by the pool
  append           cache.append(k_new, v_new) over a table the host wrote: the parent's path
  pool_fork        pool.fork(src, dst) of min(8, B / 2) sequences: fork_prepare + the fork launch
  fork             cache.fork(src, dst, new_pages) with host-chosen pages: the parent's path
  listed           sageattn_kvcache_step_listed(q, cache, cu, 1): one listed decode step
  reserve_listed   pool.reserve + the same step
Release of 1 / 8 / 32 sequences of 32 pages each (B 128), at pools of 4224 and 67584 pages: the compaction strides over every page id, so its
cost grows with the pool; raw entries over plain tensors, no cache behind them.

    python tools/kv_pool_probe.py [--rounds 5] [--reps 10] [--out profiles/kv_pool_probe.json]
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

from kv_varlen_probe import CONTEXTS, D, DISTINCT, HKV, HQ, MAX_PAGES, PAGE, time_interleaved  # noqa: E402
from sageattention_amd import _cabi_kvpool  # noqa: E402
from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache  # noqa: E402
from sageattention_amd.paged_kv_list import sageattn_kvcache_step_listed  # noqa: E402
from sageattention_amd.paged_kv_pool import PagePool  # noqa: E402
from sageattention_amd.quant import _p, _stream  # noqa: E402


class Snapshot:
    """The tensors a variant changes, and their contents now: ``restore`` puts them back (device copies on the current stream)."""

    def __init__(self, *tensors):
        self.pairs = [(t, t.clone()) for t in tensors]

    def restore(self):
        for t, saved in self.pairs:
            t.copy_(saved)


def step(B, dev):
    g = torch.Generator(device=dev).manual_seed(91 + B)
    k0, v0 = (torch.randn(DISTINCT, HKV, max(CONTEXTS), D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(2))
    k, v = k0.repeat(B // DISTINCT, 1, 1, 1), v0.repeat(B // DISTINCT, 1, 1, 1)
    km, v_amax = k.float().mean(dim=2).to(k.dtype), v.abs().float().amax(dim=2) * 2.0
    N = B * MAX_PAGES + B                      # every sequence's pages and one more each for the forks
    ints = lambda x: torch.tensor(list(x), dtype=torch.int32, device=dev)
    nf = min(8, B // 2)                        # forks: the first nf sequences into the last nf slots, which stay empty
    edge = ints(0 if b >= B - nf else CONTEXTS[b % 2] for b in range(B))            # every live sequence on a page boundary
    inner = ints(0 if b >= B - nf else CONTEXTS[b % 2] - 7 for b in range(B))       # ... and none
    pooled = PagedQuantizedKVCache.allocate(N, PAGE, B, MAX_PAGES, HKV, D, torch.bfloat16, dev)
    pooled.seed(km, v_amax)
    pool = PagePool(pooled)
    assert pool.append(k, v, inner).tolist() == inner.tolist()
    hand = PagedQuantizedKVCache.allocate(N, PAGE, B, MAX_PAGES, HKV, D, torch.bfloat16, dev)
    hand.block_table.copy_(torch.randperm(B * MAX_PAGES, generator=torch.Generator().manual_seed(B)).to(torch.int32).to(dev).view(B, MAX_PAGES))
    hand.seed(km, v_amax)
    hand.append(k, v, inner)
    del k, v, k0, v0
    k_new, v_new = (torch.randn(B, HKV, 1, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(2))
    ones = ints(0 if b >= B - nf else 1 for b in range(B))
    q = torch.randn(B, HQ, D, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    cu = ints(range(B + 1))
    src, dst, pages = ints(range(nf)), ints(range(B - nf, B)), ints(range(B * MAX_PAGES, B * MAX_PAGES + nf))
    # (filled to `inner`, seven keys in front of a page boundary: the same pages as at `edge`, where the open block and the tails are empty --
    #  an append at `edge` needs nothing of the seven rows that were never written)
    pool_inner = Snapshot(pool.ws, pooled.block_table, pooled.lens)
    hand_inner_ = Snapshot(hand.block_table, hand.lens)
    at_inner, hand_inner = pool_inner.restore, hand_inner_.restore

    def at_edge():
        pool_inner.restore()
        pooled.lens.copy_(edge)

    fns = {"reserve_idle": (at_inner, lambda: pool.reserve(new_lens=ones, T=1)),
           "reserve_pop": (at_edge, lambda: pool.reserve(new_lens=ones, T=1)),
           "pool_append": (at_inner, lambda: pool.append(k_new, v_new, ones)),
           "append": (hand_inner, lambda: hand.append(k_new, v_new, ones)),
           "pool_append_edge": (at_edge, lambda: pool.append(k_new, v_new, ones)),
           "pool_fork": (at_inner, lambda: pool.fork(src, dst)),
           "fork": (hand_inner, lambda: hand.fork(src, dst, pages)),
           "listed": (at_inner, lambda: sageattn_kvcache_step_listed(q, pooled, cu, 1)),
           "reserve_listed": (at_inner, lambda: (pool.reserve(new_lens=ones, T=1), sageattn_kvcache_step_listed(q, pooled, cu, 1)))}
    # what is timed is what the tests hold: the pool's append leaves the bytes of the hand-tabled one, the forked children attend alike
    at_inner(), hand_inner()
    pool.append(k_new, v_new, ones), hand.append(k_new, v_new, ones)
    pool.fork(src, dst), hand.fork(src, dst, pages)
    a, b = sageattn_kvcache_step_listed(q, pooled, cu, 1), sageattn_kvcache_step_listed(q, hand, cu, 1)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and bool(torch.isfinite(a.float()).all()), "the pool-managed cache attends otherwise"
    assert pool.status()["refused_total"] == 0
    return fns


def release(N, n, dev):
    """``n`` of 128 sequences of 32 pages each given back to a pool of ``N`` pages."""
    lib = _cabi_kvpool.load()
    B, mp, per = 128, MAX_PAGES, 32
    ws = torch.empty(lib.sage_kvpool_ws_bytes(N, B) // 4, dtype=torch.int32, device=dev)
    table = torch.full((B, mp), -1, dtype=torch.int32, device=dev)
    lens = torch.zeros(B, dtype=torch.int32, device=dev)
    granted = torch.empty(B, dtype=torch.int32, device=dev)
    rows = torch.full((B,), per * PAGE, dtype=torch.int32, device=dev)
    geom = (_p(ws), ws.numel() * 4, _p(table), mp, N, PAGE, mp, B)
    assert lib.sage_kvpool_init(_p(ws), ws.numel() * 4, N, B, _stream(ws)) == 0, lib.sage_last_error()
    assert lib.sage_kvpool_reserve(*geom, _p(lens), _p(rows), per * PAGE, None, 1, 1, _p(granted), _stream(ws)) == 0, lib.sage_last_error()
    lens.copy_(granted)
    assert int(ws[0]) == N - B * per and granted.tolist() == [per * PAGE] * B
    slots = torch.arange(0, B, B // n, dtype=torch.int32, device=dev)[:n].contiguous()
    full = Snapshot(ws, table, lens)

    def run():
        rc = lib.sage_kvpool_release(*geom, _p(lens), _p(slots), n, _stream(ws))
        assert rc == 0, lib.sage_last_error()
    run()
    assert int(ws[0]) == N - (B - n) * per
    return {f"release_{n}": (full.restore, run)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_pool_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kv_pool_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); bf16, D 128, Hq 32 / Hkv 8, pages of 256 keys, contexts "
                   "alternating 4096 / 8192 keys, one new row per sequence.  reserve_idle / reserve_pop = pool.reserve when no / every sequence stands on a page "
                   "boundary; pool_append = pool.append (reserve + append), append = cache.append over a host-written table (the parent's path), "
                   "pool_append_edge = pool.append with every sequence on a page boundary; pool_fork = pool.fork of min(8, B / 2) sequences, fork = cache.fork "
                   "with host-chosen pages; listed = one listed decode step, reserve_listed = pool.reserve + that step.  release: n of 128 sequences of 32 pages "
                   "given back to a pool of num_pages pages.  spread = range of the round medians / the figure; x_over_y = ratio of the figures of the same run",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "step": [], "release": []}
    pairs = (("pool_append", "append"), ("pool_append_edge", "append"), ("pool_fork", "fork"), ("reserve_listed", "listed"), ("reserve_idle", "listed"))

    def figures(per_round):
        r = {}
        for n, xs in per_round.items():
            med = statistics.median(xs)
            r[n] = {"us": round(med, 1), "spread": round((max(xs) - min(xs)) / med, 4), "us_rounds": [round(x, 1) for x in xs]}
        return r

    for B in (4, 32, 128):
        fns = step(B, dev)
        r = dict({"B": B}, **figures(time_interleaved(fns, a.rounds, a.reps)))
        for x, y in pairs:
            r[f"{x}_over_{y}"] = round(r[x]["us"] / r[y]["us"], 4)
            r[f"{x}_minus_{y}_us"] = round(r[x]["us"] - r[y]["us"], 1)
        res["step"].append(r)
        print(f"B {B:3d}: " + "  ".join(f"{n} {r[n]['us']:7.1f} us (+-{100 * r[n]['spread']:.1f}%)" for n in fns), flush=True)
        del fns
        torch.cuda.empty_cache()
    for N in (4224, 67584):
        fns = {}
        for n in (1, 8, 32):
            fns.update(release(N, n, dev))
        r = dict({"num_pages": N}, **figures(time_interleaved(fns, a.rounds, a.reps)))
        res["release"].append(r)
        print(f"release, {N} pages: " + "  ".join(f"{n} {r[n]['us']:7.1f} us (+-{100 * r[n]['spread']:.1f}%)" for n in fns), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
