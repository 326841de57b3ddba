"""GPU: seeded random PROGRAMS of cache operations on the quantised KV-cache family, held step by step to a page-free model.

The feature files of the cache hold each route to the sibling added just before it (packed = dense paged = contiguous = the one-shot call), on a
freshly built cache seeded with the statistics of its own final content.  Here a program (``ref_kvcache_sim.random_program``, ``SAGE_PROGRAM_SEEDS``
seeds, default 40) composes the features the way a continuous-batching engine does -- slots seeded from a prompt with head-room and appended to
for long afterwards, dense and packed appends, forks of whole parents and of prefixes, different rows to parent and child, slots released and
seeded again through recycled pages that still hold another sequence's bytes, appends past the capacity, saturating V rows -- and after EVERY step
the GPU is compared with tests/ref_kvcache_sim.py, which knows nothing of the kernels:

  * after every mutating step all ten cache tensors equal the simulator's, byte for byte -- the tail rows at or behind ``lens % 64`` included (an
    append writes the tail rows it opens and no others, a fork copies the rows in front of ``P % 64``, and the simulator follows both, so nothing
    is masked); the keys every slot's table serves are the ledger's operands; pages the allocator never handed out keep their poison.  The
    message names the tensor, the pages or slots, and the step;
  * after every attention step -- one call over all slots -- each slot is checked against ``ref_window.attn_window`` on the LEDGER's operands
    (not the bytes read back from the GPU), under ``ref_window.visible_from_keywords`` with the public meaning of the keywords (bottom-right:
    ``q_start = lens[b] - Lq_b``), Q quantised by the oracle, the LSE with the slot's ``q . k_mean`` correction
    (test_gpu_route_tile_counts.py::check_sample_quantised), at the project's bars: ``2e-3 max|ref| + 2`` output ulps, LSE within 5e-3, rows
    without keys exactly +0 / -inf where the predicate says so.  Rows of a packed call that no slot owns keep their poison;
  * the route equalities the project promises, where they are drawn: a ``pack_gqa`` call equals its unpacked twin bit for bit; a packed-varlen
    slot equals the dense call of its rows (bottom-right, or the same ``q_start``; the same window) bit for bit.

The first 10 seeds run once more on a contiguous ``QuantizedKVCache`` with the fork, packed and paging operations filtered out
(``ref_kvcache_sim.contiguous_variant``), judged through the ledger and the attention reference alone.

Shapes (the smallest at which every branch is reachable): 6 slots, Hkv 2, group 1 / 4, D 64 / 128, fp16 / bf16, smooth_k on / off, pages of 64 /
128 / 256 keys with a logical capacity of 512, a poisoned pool dealt out in a fixed permutation, unneeded table entries -1 and num_pages in turn.
What the generator reaches is asserted on the CPU (tests/test_kvcache_sim_host.py, part c), where the simulator is also proved against the ledger
on 200 programs and five deliberately wrong caches are each reported.

Not drawn: a channel with ``v_amax == 0`` (the ledger defines its bytes as 0; the sign of a zero product is not what this file is about), ids
outside the pool, malformed prefix arrays, graphs and streams -- test_gpu_fence.py and the feature files keep those.

Measured on an MI355X over the 40 default seeds (344 mutating steps, 132 attention steps; every byte comparison and every bar held, no kernel
changed) -- per attention route the largest ``err / bar`` and the largest LSE error of any slot; each test prints its own:

    route                                                          err / bar   lse
    sageattn_kvcache, non-causal                                   0.410       3.1e-05
    sageattn_kvcache, causal top-left                              0.209       7.6e-06
    sageattn_kvcache, causal bottom-right                          0.409       1.9e-06
    sageattn_kvcache, q_start tensor                               0.220       3.5e-04
    sageattn_kvcache, window_size=(W, 0)                           0.435       1.9e-06
    sageattn_kvcache, pack_gqa (= its unpacked twin, bit for bit)  0.403       1.9e-06
    sageattn_kvcache_split, S 2 / 3 / 8                            0.204       1.9e-06
    sageattn_kvcache_varlen (= the dense call, bit for bit)        0.421       2.4e-06
    sageattn_kvcache_varlen, window_size=(W, 0)                    0.402       6.1e-05
    sageattn_kvcache_varlen, q_start tensor                        0.218       3.4e-04

The slowest seed takes 0.64 s (seed 0, which also pays the process's first launches; the next is 0.34 s), the whole file 10 s.
"""
import os
import time

import numpy as np
import pytest
import torch

import ref_kvcache_sim as sim
import ref_window as rw
import util
from fence import Fence
from test_gpu_route_tile_counts import check_sample_quantised

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi
    from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    from sageattention_amd.paged_kv_split import sageattn_kvcache_split
    from sageattention_amd.paged_kv_varlen import append_varlen, sageattn_kvcache_varlen
    DEV = torch.device("cuda:0")

SEEDS = int(os.environ.get("SAGE_PROGRAM_SEEDS", "40"))
CONTIGUOUS_SEEDS = 10
NSLOTS, HKV = sim.NSLOTS, sim.HKV
WORST = {}                          # route -> [largest err / bar, largest LSE error], over the session (printed by every test)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _ints(values, dtype=torch.int32):
    return torch.tensor([int(x) for x in values], dtype=dtype, device=DEV)


def _t(bits, code):
    return util.from_bits(bits, code, DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _new_cache(shape, run, contiguous):
    """The cache under test: every byte poisoned, the program's first table, the whole cache seeded with the run's first statistics."""
    dt = torch.float16 if shape["code"] == 0 else torch.bfloat16
    if contiguous:
        c = QuantizedKVCache.allocate(NSLOTS, HKV, sim.CAP, shape["D"], dt, DEV)
    else:
        c = PagedQuantizedKVCache.allocate(shape["num_pages"], shape["page_size"], NSLOTS, shape["max_pages"], HKV, shape["D"], dt, DEV)
        c.block_table.copy_(_ints(shape["table"]).view(NSLOTS, -1))
    for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.v_amax, c.k_mean, c.k_tail, c.v_tail):
        t.view(torch.uint8).fill_(sim.POISON)
    c.seed(None if run.km0 is None else _t(run.km0, shape["code"]), torch.from_numpy(run.va0).to(DEV))
    return c


def _state(c):
    """The cache's ten tensors as ref_kvcache_sim takes them (integer views on the host); a contiguous cache: one page per slot, the identity table."""
    i = lambda t, dt: t.contiguous().view(dt).cpu().numpy()
    table = c.block_table.cpu().numpy() if hasattr(c, "block_table") else np.arange(NSLOTS, dtype=np.int32).reshape(NSLOTS, 1)
    return dict(k_int8=c.k_int8.cpu().numpy(), k_scale=i(c.k_scale, torch.int32), v_image=c.v_image.cpu().numpy(), v_scale=i(c.v_scale, torch.int32),
                v_amax=i(c.v_amax, torch.int32), k_mean=None if c.k_mean is None else i(c.k_mean, torch.int16), k_tail=i(c.k_tail, torch.int16),
                v_tail=i(c.v_tail, torch.int16), lens=c.lens.cpu().numpy(), block_table=table)


def _seed_slots(c, act, code, contiguous):
    km = None if act["k_mean"] is None else _t(act["k_mean"], code)
    va = torch.from_numpy(act["v_amax"]).to(DEV)
    if contiguous:
        c._seed(km, va, _ints(act["slots"], torch.int64))
    else:
        c.seed(km, va, slots=list(act["slots"]))


def _mutate(c, act, code, contiguous):
    """One mutating step on the GPU cache: the table entries its caller writes, then the call."""
    op = act["op"]
    if act["table"]:
        rows = torch.tensor([b for b, _, _ in act["table"]], device=DEV)
        cols = torch.tensor([e for _, e, _ in act["table"]], device=DEV)
        c.block_table[rows, cols] = _ints([p for _, _, p in act["table"]])
    if op in ("prefill", "reseed"):
        _seed_slots(c, act, code, contiguous)
    if op == "append" or (op == "prefill" and not act["packed"]):
        new_lens = act["new_lens"] if op == "append" else act["counts"]
        dtype = torch.int64 if op == "append" and act["i64"] else torch.int32
        c.append(_t(act["k"], code), _t(act["v"], code), None if new_lens is None else _ints(new_lens, dtype))
    elif op == "append_varlen" or op == "prefill":
        append_varlen(c, _t(act["k"], code), _t(act["v"], code), _ints(act["cu"]), act["max_new"])
    elif op == "fork":
        wrap = {None: lambda x: list(x), "i32": lambda x: _ints(x), "i64": lambda x: _ints(x, torch.int64)}[act["tensors"]]
        c.fork(wrap(act["src"]), wrap(act["dst"]), wrap(act["pages"]), None if act["prefix"] is None else wrap(act["prefix"]))
    torch.cuda.synchronize()


def _dense_kw(step):
    kw = dict(return_lse=True)
    mask = step["align"] if step["mask"] == "window" else step["mask"]
    if step["mask"] != "nc":
        kw["is_causal"] = True
    if mask == "br":
        kw["causal_align"] = "bottom_right"
    elif mask == "qstart":
        kw["q_start"] = _ints(step["q_start"])
    if step["window"] is not None:
        kw["window_size"] = (step["window"], 0)
    return kw


def _attend(c, act, code):
    """The attention call of one step over all slots; per slot (o float32 [Hq, Lq_b, D], lse float32 [Hq, Lq_b]) on the host.  The promised
    route equalities are asserted here."""
    step, D = act, c.D
    if not step["route"].startswith("varlen"):
        q = _t(act["q"], code)                                                   # [B, Hq, Lq, D]
        kw = _dense_kw(step)
        if step["route"] == "split":
            o, lse = sageattn_kvcache_split(q, c, step["splits"], pack_gqa=step["pack"], **kw)
            twin = (lambda: sageattn_kvcache_split(q, c, step["splits"], pack_gqa=False, **kw)) if step["pack"] else None
        else:
            o, lse = sageattn_kvcache(q, c, pack_gqa=step["pack"], **kw)
            twin = (lambda: sageattn_kvcache(q, c, pack_gqa=False, **kw)) if step["pack"] else None
        assert o.shape == q.shape and lse.shape == q.shape[:3]
        if twin is not None:
            o2, lse2 = twin()
            assert torch.equal(_bits(o), _bits(o2)), f"the pack_gqa call's o differs from its unpacked twin in {int((_bits(o) != _bits(o2)).sum())} elements"
            assert torch.equal(_bits(lse), _bits(lse2)), f"the pack_gqa call's lse differs from its unpacked twin in {int((_bits(lse) != _bits(lse2)).sum())} rows"
        torch.cuda.synchronize()
        o, lse = o.float().cpu().numpy(), lse.cpu().numpy()
        return [(o[b], lse[b]) for b in range(NSLOTS)]
    counts, cu, total = step["counts"], act["cu"], act["total"]
    q = _t(act["q"], code)                                                       # [total, Hq, D]
    kw = {}
    if step["window"] is not None:
        kw["window_size"] = (step["window"], 0)
    if step["q_start"] is not None:
        kw["q_start"] = _ints(step["q_start"])
    with Fence(sim.POISON) as f:                                                 # (o and lse are the package's torch.empty: poisoned bodies between guards)
        o, lse = sageattn_kvcache_varlen(q, c, _ints(cu), max(counts), return_lse=True, **kw)
        f.check()
        o, lse = o.clone(), lse.clone()
    assert o.shape == q.shape and lse.shape == (q.shape[1], total)
    nobody = torch.cat((o[:cu[0]], o[cu[-1]:])).contiguous().view(torch.uint8)
    assert bool((nobody == sim.POISON).all()), "rows of o that no slot owns were written"
    # a packed slot is the dense call of its rows: bottom-right or the same q_start, the same window -- bit for bit
    for L in sorted(set(counts) - {0}):
        qd = torch.zeros(NSLOTS, L, q.shape[1], D, dtype=q.dtype, device=DEV)
        for b, n in enumerate(counts):
            if n == L:
                qd[b] = q[cu[b]:cu[b + 1]]
        dkw = dict(kw, is_causal=True, return_lse=True, tensor_layout="NHD")
        if step["q_start"] is None:
            dkw["causal_align"] = "bottom_right"
        od, ld = sageattn_kvcache(qd, c, **dkw)
        for b, n in enumerate(counts):
            if n == L:
                do, dl = _bits(o[cu[b]:cu[b + 1]]) != _bits(od[b]), _bits(lse[:, cu[b]:cu[b + 1]]) != _bits(ld[b])
                assert not bool(do.any()), f"slot {b} (Lq {L}): o of the packed call differs from the dense call in {int(do.sum())} of {do.numel()} elements"
                assert not bool(dl.any()), f"slot {b} (Lq {L}): lse of the packed call differs from the dense call in {int(dl.sum())} of {dl.numel()} rows"
    torch.cuda.synchronize()
    o, lse = o.float().cpu().numpy(), lse.cpu().numpy()
    return [(np.ascontiguousarray(o[cu[b]:cu[b + 1]].transpose(1, 0, 2)), lse[:, cu[b]:cu[b + 1]]) for b in range(NSLOTS)]


def _check_attention(oracle, tag, run, act, code, got):
    """Each slot against the reference on the ledger's operands."""
    led, D = run.ledger, run.D
    Hq = HKV * run.shape["group"]
    for b in range(NSLOTS):
        L = led.length(b)
        Lq, window, causal, start = sim.attn_geometry(act, b, L)
        if act["route"].startswith("varlen"):
            q_bits = np.ascontiguousarray(act["q"][act["cu"][b]:act["cu"][b + 1]].transpose(1, 0, 2))
        else:
            q_bits = act["q"][b]
        assert q_bits.shape == (Hq, Lq, D) and got[b][0].shape == (Hq, Lq, D) and got[b][1].shape == (Hq, Lq)
        if Lq == 0:
            continue
        ops = led.operands(b)
        keep = rw.visible_from_keywords(Lq, L, window, causal, start, L)
        ratio, lerr = check_sample_quantised(oracle, f"{tag} slot {b} (len {L}, Lq {Lq}, offset {start}, window {window})", q_bits, ops["K8"], ops["k_scale"],
                                             ops["V8"], ops["v_scale"], led.k_mean[b], code, D, keep, got[b][0], got[b][1])
        worst = WORST.setdefault(act["route"], [0.0, 0.0])
        worst[0], worst[1] = max(worst[0], ratio), max(worst[1], lerr)


def _run_program(oracle, seed, contiguous):
    shape, steps = sim.random_program(seed)
    if contiguous:
        shape, steps = sim.contiguous_variant(shape, steps)
    code = shape["code"]
    run = sim.Run(oracle, shape, steps)
    c = _new_cache(shape, run, contiguous)
    print(f"seed {seed}{' contiguous' if contiguous else ''}: " + " ".join(f"{k}={shape[k]}" for k in ("D", "code", "smooth_k", "group", "page_size")) +
          f", {len(steps)} steps: " + " ".join(s["op"] if s["op"] != "attn" else s["route"] for s in steps))
    t0 = time.time()
    for i, step in enumerate(steps):
        act = run.action(i)
        what = f"seed {seed} step {i} ({step['op'] if step['op'] != 'attn' else step['route']})"
        if step["op"] == "attn":
            _check_attention(oracle, what, run, act, code, _attend(c, act, code))
            continue
        _mutate(c, act, code, contiguous)
        run.advance(i, act)
        got = _state(c)
        bad = sim.logical_mismatches(got, shape["page_size"], run.ledger, range(NSLOTS))
        if not contiguous:
            bad = sim.state_mismatches(got, run.state) + bad + sim.untouched_pages_mismatches(got, step["handed"])
        assert not bad, f"{what}: " + "; ".join(bad[:6])
        assert got["lens"].tolist() == step["lens"], (what, got["lens"].tolist(), step["lens"])
    print(f"TIME seed {seed}{' contiguous' if contiguous else ''}: {time.time() - t0:.2f} s")
    for route in sorted(WORST):
        print(f"WORST so far {route}: err / bar {WORST[route][0]:.3f}, lse {WORST[route][1]:.2e}")


@pytest.mark.parametrize("seed", list(range(SEEDS)))
def test_random_programs_on_the_paged_cache(oracle_mod, seed):
    _run_program(oracle_mod, seed, False)


@pytest.mark.parametrize("seed", list(range(CONTIGUOUS_SEEDS)))
def test_random_programs_on_the_contiguous_cache(oracle_mod, seed):
    _run_program(oracle_mod, seed, True)
