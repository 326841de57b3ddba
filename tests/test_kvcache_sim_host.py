"""CPU: the two layers of tests/ref_kvcache_sim.py hold each other, the program generator reaches what tests/test_gpu_kvcache_programs.py relies
on, and the comparison functions that file asserts with report wrong caches.

  a  the ledger is pinned to the oracle: seeded with the content's own ``channel_mean`` and exact abs-max, its K8 / k_scale / V8 / v_scale are
     ``oracle.quant_int8`` and ``oracle.quant_v_fp8(scale_max=448)`` on the same rows, byte for byte (the V conversion of the ledger is written
     from the e4m3 format; here it meets the oracle's converter, on every rounding boundary too), and the attention reference the GPU file
     uses on such operands (test_gpu_route_tile_counts.py::ref_sample_quantised) is the oracle's causal path on the raw rows;
  b  the simulator agrees with the ledger: the first 200 programs, after every mutating step ``logical(state, b)`` is the ledger's operands
     for every slot, the lengths are the program's plan, and every pool page the allocator never handed out is still all poison;
  c  the generator's conditions over the GPU test's default seeds (the counts are printed);
  d  five wrong caches (``ref_kvcache_sim.MUTANTS``) are each reported within the first 20 seeds, the unmutated simulator never.
"""
import collections

import numpy as np
import pytest

import ref_kvcache_sim as sim
import util

DEFAULT_SEEDS = 40            # tests/test_gpu_kvcache_programs.py: SAGE_PROGRAM_SEEDS


# ---- a ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", (0, 1), ids=("f16", "bf16"))
@pytest.mark.parametrize("D", (64, 128))
def test_a_the_ledger_is_the_oracles_quantisers(oracle_mod, D, code):
    O, H = oracle_mod, 2
    for L in (1, 63, 64, 65, 257):
        rng = np.random.default_rng([5, D, code, L])
        k = sim.to_bits(rng.standard_normal((1, H, L, D)).astype(np.float32) + 1.5 * rng.standard_normal((1, H, 1, D)).astype(np.float32), code)
        v = sim.to_bits(rng.standard_normal((1, H, L, D)).astype(np.float32) * (0.25 + rng.random((1, H, 1, D))).astype(np.float32), code)
        km = O.k_mean(k, code)                                                    # [1, H, D]: the content's own channel mean, in the input dtype
        v_amax = np.abs(util.f32(v, code)).max(axis=2)                            # exact
        led = sim.Ledger(O, 1, H, D, code, 512)
        led.seed([0], km, v_amax)
        cuts = sorted({0, L // 3, L // 2, L})                                     # (appended in pieces: the ledger is free of blocks)
        for a, b in zip(cuts, cuts[1:]):
            led.append(0, k[0, :, a:b], v[0, :, a:b])
        got = led.operands(0)
        gk, nk = O.group_index(L, "per_thread", "k", 64, 64)
        k8, ks = O.quant_int8(k, code, gk, nk, style=O.STYLE_TRITON_THREAD, mean=km)
        v8, vs = O.quant_v_fp8(v, code, scale_max=448.0)
        assert got["K8"].dtype == np.int8 and np.array_equal(got["K8"], k8[0]), (L, "K8")
        assert np.array_equal(got["k_scale"].view(np.uint32), ks[0].view(np.uint32)), (L, "k_scale")
        assert np.array_equal(got["V8"], v8[0]), (L, "V8", int((got["V8"] != v8[0]).sum()))
        assert np.array_equal(got["v_scale"].view(np.uint32), vs[0].view(np.uint32)), (L, "v_scale")


def test_a_the_e4m3_conversion_of_every_rounding_boundary(oracle_mod):
    """The ledger's converter against the oracle's on every e4m3 value, every midpoint between neighbours, and one fp32 step to either side."""
    vals = np.sort(np.unique(np.abs(oracle_mod.e4m3_to_f32(np.arange(256, dtype=np.uint8))[np.r_[0:0x7F, 0x80:0xFF]])))
    mids = (vals[:-1].astype(np.float64) + vals[1:].astype(np.float64)) / 2
    pts = np.concatenate((vals, mids.astype(np.float32), np.array([456.0, 464.0, 480.0, 1e6, 2.0 ** -11, 2.0 ** -12], np.float32)))
    pts = np.concatenate((pts, np.nextafter(pts, np.float32(0)), np.nextafter(pts, np.float32(np.inf)))).astype(np.float32)
    pts = np.concatenate((pts, -pts))
    assert np.array_equal(sim.e4m3_rne(pts), oracle_mod.convert(pts, "e4m3"))


@pytest.mark.parametrize("D,code", [(64, 0), (128, 1)])
def test_a_the_attention_reference_on_ledger_operands_is_the_oracles_causal_path(oracle_mod, D, code):
    """``test_gpu_route_tile_counts.ref_sample_quantised`` on the operands of a ledger seeded with its content's own statistics against
    ``oracle.sageattn_dense`` (FP8 PV, per-thread, causal, top-left) on the raw rows, under test_second_restatement.py's criterion, which
    test_window_host.py holds ``ref_window.attn_window`` to: o within one output ulp on fewer than 2e-3 of the elements, lse within 2e-6
    max(1, max|lse|)."""
    import ref_window as rw
    from test_gpu_route_tile_counts import ref_sample_quantised
    O, H, Hq, L, Lq = oracle_mod, 2, 4, 130, 40
    rng = np.random.default_rng([6, D, code])
    q = sim.to_bits(rng.standard_normal((1, Hq, Lq, D)).astype(np.float32), code)
    k = sim.to_bits(rng.standard_normal((1, H, L, D)).astype(np.float32) + 1.5 * rng.standard_normal((1, H, 1, D)).astype(np.float32), code)
    v = sim.to_bits(rng.standard_normal((1, H, L, D)).astype(np.float32), code)
    km = O.k_mean(k, code)
    led = sim.Ledger(O, 1, H, D, code, 512)
    led.seed([0], km, np.abs(util.f32(v, code)).max(axis=2))
    led.append(0, k[0], v[0])
    ops = led.operands(0)
    keep = rw.visible_from_keywords(Lq, L, (-1, -1), True, 0, L)
    o, lse = ref_sample_quantised(O, q[0], ops["K8"], ops["k_scale"], ops["V8"], ops["v_scale"], km[0], code, D, keep)
    want, lse_want, _ = O.sageattn_dense(q, k, v, code, is_causal=True, pv="f8", qk_quant_gran="per_thread", return_lse=True, km=km, fp8_scores="exact")
    diff = np.abs(sim.to_bits(o, code).astype(np.int32) - want[0].astype(np.int32))
    lerr = float(np.abs(lse - lse_want[0]).max())
    print(f"D {D} code {code}: {float((diff != 0).mean()):.2e} of the outputs differ (max {int(diff.max())} ulp), lse {lerr:.2e}")
    assert diff.max() <= 1 and (diff != 0).mean() < 2e-3
    assert lerr <= 2e-6 * max(1.0, float(np.abs(lse_want).max()))


# ---- b ----------------------------------------------------------------------------------------------------------------------------------
def _walk(oracle, seed, mutant=None, contiguous=False):
    """Program ``seed`` step by step: yields (i, step, act, run) after each mutating step has been applied."""
    shape, steps = sim.random_program(seed)
    if contiguous:
        shape, steps = sim.contiguous_variant(shape, steps)
    run = sim.Run(oracle, shape, steps, mutant)
    for i, step in enumerate(steps):
        act = run.action(i)
        if step["op"] != "attn":
            run.advance(i, act)
            yield i, step, act, run


@pytest.mark.parametrize("chunk", range(8))
def test_b_the_simulator_agrees_with_the_ledger(oracle_mod, chunk):
    steps = 0
    for seed in range(25 * chunk, 25 * chunk + 25):
        for i, step, _, run in _walk(oracle_mod, seed):
            bad = run.check(i)
            assert not bad, f"seed {seed}: " + "; ".join(bad[:4])
            steps += 1
    print(f"programs {25 * chunk} .. {25 * chunk + 24}: {steps} mutating steps")


def test_b_the_contiguous_variant_agrees_with_the_ledger(oracle_mod):
    for seed in range(10):
        for i, step, _, run in _walk(oracle_mod, seed, contiguous=True):
            assert step["op"] not in ("fork", "append_varlen")
            bad = run.check(i)
            assert not bad, f"seed {seed}: " + "; ".join(bad[:4])


# ---- c ----------------------------------------------------------------------------------------------------------------------------------
def _fork_then_both_then_attention(steps):
    """A fork, later appends that give rows to its parent and to its child (while neither is seeded again), an attention step behind them."""
    for i, f in enumerate(steps):
        if f["op"] != "fork":
            continue
        s, d = f["src"][0], f["dst"][0]
        got_s = got_d = False
        for step in steps[i + 1:]:
            if step["op"] in ("append", "append_varlen"):
                got_s, got_d = got_s or step["given"][s] > 0, got_d or step["given"][d] > 0
            elif step["op"] in ("prefill", "reseed") and {s, d} & set(step["rows"] if step["op"] == "prefill" else step["slots"]):
                break
            elif step["op"] == "fork" and {s, d} & set(step["dst"]):
                break
            elif step["op"] == "attn" and got_s and got_d:
                return True
    return False


def _rows_that_see_a_key(step, b, L):
    Lq, (left, _), causal, start = sim.attn_geometry(step, b, L)
    n = 0
    for i in range(Lq):
        hi = min(L - 1, start + i) if causal else L - 1
        lo = max(0, start + i - left) if left >= 0 else 0
        n += hi >= lo
    return n, Lq


def test_c_the_generators_conditions():
    ops, routes, shapes = collections.Counter(), collections.Counter(), collections.Counter()
    composed = dry = attn = attn_live = 0
    for seed in range(DEFAULT_SEEDS):
        shape, steps = sim.random_program(seed)
        assert 10 <= len(steps) <= 14 and steps[-1]["op"] == "attn"
        dry += shape["dry"]
        composed += _fork_then_both_then_attention(steps)
        for key in ("page_size", "D", "code", "smooth_k", "group"):
            shapes[key, shape[key]] += 1
        lens = [0] * sim.NSLOTS
        for step in steps:
            if step["op"] != "attn":
                ops[step["op"]] += 1
                ops["overflow"] += bool(step["overflow"])
                ops["saturating"] += step["sat"] is not None
                if step["op"] == "fork":
                    ops["fork_prefix"] += step["prefix"] is not None
                    ops["fork_whole"] += step["prefix"] is None
                lens = step["lens"]
                continue
            routes[step["route"]] += 1
            attn += 1
            seen = [_rows_that_see_a_key(step, b, lens[b]) for b in range(sim.NSLOTS)]
            attn_live += any(lq > 0 and 2 * n >= lq for n, lq in seen)
    print("operations:", dict(ops))
    print("attention routes:", dict(routes))
    print("shapes:", dict(shapes))
    print(f"fork -> appends to parent and child -> attention: {composed} of {DEFAULT_SEEDS} programs; attention steps with a slot in which at "
          f"least half the rows see a key: {attn_live} of {attn}; programs in which the allocator runs dry: {dry}")
    for kind in sim.MUTATING + ("overflow", "saturating", "fork_prefix", "fork_whole"):
        assert ops[kind] >= 5, (kind, ops[kind])
    for route in sim.ROUTES:
        assert routes[route] >= 5, (route, routes[route])
    assert composed >= 0.6 * DEFAULT_SEEDS, composed
    assert attn_live >= 0.9 * attn, (attn_live, attn)
    assert dry == 0
    for key, values in (("page_size", sim.PAGE_SIZES), ("D", (64, 128)), ("code", (0, 1)), ("smooth_k", (False, True)), ("group", (1, 4))):
        assert all(shapes[key, v] > 0 for v in values), (key, shapes)


def test_c_a_program_is_the_same_program_every_time():
    assert sim.random_program(7) == sim.random_program(7) and sim.random_program(7)[1] != sim.random_program(8)[1]


# ---- d ----------------------------------------------------------------------------------------------------------------------------------
def _reports(oracle, seed, mutant):
    """What part 3's comparisons say about a cache that behaves as ``mutant`` on program ``seed``: the mutated simulator plays the device, the
    unmutated one is what it is held to after every mutating step, byte for byte in all ten tensors; the ledger judges the keys it serves."""
    shape, steps = sim.random_program(seed)
    truth, device = sim.Run(oracle, shape, steps), sim.Run(oracle, shape, steps, mutant)
    for i, step in enumerate(steps):
        if step["op"] == "attn":
            continue
        act = truth.action(i)
        truth.advance(i, act)
        device.advance(i, act)
        found = sim.state_mismatches(device.state, truth.state) + sim.logical_mismatches(device.state, shape["page_size"], truth.ledger, range(sim.NSLOTS))
        if found:
            return [f"seed {seed} step {i} ({step['op']}): {m}" for m in found]
    return []


@pytest.mark.parametrize("mutant", sim.MUTANTS)
def test_d_a_wrong_cache_is_reported(oracle_mod, mutant):
    for seed in range(20):
        found = _reports(oracle_mod, seed, mutant)
        if found:
            print(f"{mutant}: " + found[0])
            assert any(name in found[0] for name in sim.KEYS + ("K8", "V8")) and "step" in found[0]
            return
    raise AssertionError(f"{mutant}: not reported within 20 seeds")


def test_d_the_unmutated_simulator_is_not_reported(oracle_mod):
    for seed in range(20):
        assert _reports(oracle_mod, seed, None) == []
