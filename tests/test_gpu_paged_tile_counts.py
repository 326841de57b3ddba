"""GPU: tile-count sweep of the six paged compilation units -- ``*_f8p`` (the kv_lens / q_start / window forms behind a block table), ``*_f8pg``
(``pack_gqa``), ``*_f8pks`` (pass 2 of the exact split), ``*_f8pr`` (packed query rows), ``*_f8pb`` and ``*_f8pbg`` (the step call's chunk and
decode launches), at D 64 and D 128.

Each unit compiles the hand-scheduled six-body loop (csrc/sage_attn_loop_f8.h) on its own, with a block-table lookup and a scalar load of the
page id added per tile, and the feature tests of the paged cache stop at 640 .. 1061 keys: mostly a single trip of the six-body loop and few of
its remainders.  Here the logical capacity is 1536 keys (24 tiles; 2560 for the split, where a chunk of S = 2 holds 20) and the lengths, offsets,
windows and row counts are CHOSEN with ``loop_plan`` -- the host model of a work item's loop partition -- so that every unit runs 0, 1 and 2
trips with every remainder 0 .. 5, behind the last-tile bodies and in front of both kinds of diagonal, with 0 .. 3 head tiles of a window in
front.  What the tables reach is asserted on the CPU in tests/test_paged_tile_counts_host.py; a failing comparison here names the samples that
differ with the model's forms of their query blocks.

ONE cache per (D, dtype, page size) serves every unsplit route: sample b holds ``lp.PAGED_SAMPLES[b][0]`` keys and every causal call places its
row 0 at ``lp.PAGED_SAMPLES[b][1]``; a windowed call is one W over all samples.  Pages of 64 keys (a page boundary behind every tile) and of 256
(behind every fourth; with S 3 a chunk starts inside a page), Hkv 2, groups 1 / 4 / 5, fp16 and bf16; the table is an interleaved, non-ascending
permutation over a poisoned pool of twice the need, with -1 / num_pages / 2^31 - 1 in the entries no tile needs.  The caches are built once at
module scope and no test modifies them.

References -- the chain's own, no tolerance:
  * paged == the contiguous ``QuantizedKVCache`` of the same appended content and statistics: ``o`` and ``lse`` bit for bit, and for the split
    the workspace (chunk maxima, partial LSEs and outputs, padding) byte for byte through the C entries;
  * ragged == the dense paged call of each sequence's rows, bit for bit;
  * step == ragged, bit for bit on the rows a sequence owns, poison elsewhere (tests/test_gpu_kv_step.py::_assert_same).
So that the chain cannot float as a whole, one sample per unit and D with at least two trips and a remainder is held to
``ref_window.attn_window`` on the LEDGER's operands (tests/ref_kvcache_sim.py: the oracle's quantiser on the raw rows, nothing read back from
the GPU) at the bars of tests/test_gpu_kvcache_programs.py: ``2e-3 max|ref| + 2`` output ulps, LSE within 5e-3.
"""
import copy
import functools
import random

import numpy as np
import pytest
import torch

import loop_plan as lp
import ref_kvcache_sim as sim
import ref_window as rw
import util
from test_gpu_kv_step import _assert_same
from test_gpu_paged_kv import _bits_equal, _table
from test_gpu_route_tile_counts import check_sample_quantised

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sageattention_amd import _cabi, _cabi_kvpsplit, core as sc, quant as sq
    from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    from sageattention_amd.paged_kv_split import sageattn_kvcache_split
    from sageattention_amd.paged_kv_step import sageattn_kvcache_step
    from sageattention_amd.paged_kv_varlen import sageattn_kvcache_varlen
    DEV = torch.device("cuda:0")

HKV = lp.PAGED_HKV
POISON = 0x5A
F16, BF16 = torch.float16, torch.bfloat16
CASES = [(64, F16), (64, BF16), (128, F16), (128, BF16)]
CASE_IDS = [f"d{D}-{'f16' if dt == F16 else 'bf16'}" for D, dt in CASES]
PAGES = lp.PAGED_PAGE_SIZES
PAGE_IDS = [f"page{p}" for p in PAGES]
# (name, samples, logical capacity)
TABLES = {"main": (lp.PAGED_SAMPLES, lp.LKP), "split": (lp.paged_split_samples(), lp.LKP_SPLIT)}
MAX_ROWS = max(lp.PAGED_RAGGED_LQS)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()
    yield
    for f in (_content, _caches, _q, _rows):
        f.cache_clear()
    torch.cuda.empty_cache()


def _ints(values):
    return torch.tensor([int(x) for x in values], dtype=torch.int64).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).to(DEV)


def _u8(t):
    return t.contiguous().view(torch.uint8)


def _lens(which):
    samples, cap = TABLES[which]
    return [min(max(n, 0), cap) for n, _ in samples]


@functools.lru_cache(maxsize=None)
def _content(D, dt, which):
    """k, v ``[nb, HKV, cap, D]`` (HND) with a per-channel K bias, the K mean and the V abs-max of each sample's valid rows: made once, never
    modified."""
    samples, cap = TABLES[which]
    nb = len(samples)
    g = torch.Generator().manual_seed(71 + D + cap)
    k = (torch.randn(nb, HKV, cap, D, generator=g) + 1.5 * torch.randn(1, HKV, 1, D, generator=g)).to(dt).to(DEV)
    v = (torch.randn(nb, HKV, cap, D, generator=g) * (0.25 + torch.rand(1, HKV, 1, D, generator=g))).to(dt).to(DEV)
    lens = _ints(_lens(which))
    valid = (torch.arange(cap, device=DEV)[None, :] < lens[:, None]).view(nb, 1, cap, 1)
    v_amax = torch.where(valid, v.abs().float(), 0.0).amax(dim=2)
    return k, v, sq.channel_mean_kvlens(k, lens, "HND"), v_amax, lens


@functools.lru_cache(maxsize=None)
def _caches(D, dt, page_size, which):
    """(contiguous cache, poisoned paged cache) of one content, one set of statistics and one append: built once, shared, never modified."""
    samples, cap = TABLES[which]
    nb, lens_h = len(samples), _lens(which)
    k, v, km, v_amax, lens = _content(D, dt, which)
    max_pages = cap // page_size
    num_pages = 2 * sum((n + page_size - 1) // page_size for n in lens_h)
    perm = random.Random(page_size + D).sample(range(num_pages), num_pages)
    table = _table(lens_h, page_size, max_pages, perm, num_pages)
    ref = QuantizedKVCache.allocate(nb, HKV, cap, D, dt, DEV)
    c = PagedQuantizedKVCache.allocate(num_pages, page_size, nb, max_pages, HKV, D, dt, DEV)
    for t in (c.k_int8, c.k_scale, c.v_image, c.v_scale, c.k_tail, c.v_tail):
        t.view(torch.uint8).fill_(POISON)
    c.block_table.copy_(torch.tensor(table, dtype=torch.int64).to(torch.int32).to(DEV))
    for cache in (ref, c):
        cache.seed(km, v_amax)
        cache.append(k, v, lens)
    torch.cuda.synchronize()
    assert ref.capacity == c.capacity == cap and ref.lens.tolist() == c.lens.tolist() == lens_h
    used = [p for b, n in enumerate(lens_h) for p in table[b][:(n + page_size - 1) // page_size]]
    assert len(set(used)) == len(used) and all(0 <= p < num_pages for p in used) and sorted(table[-1][:4]) != table[-1][:4]
    return ref, c


@functools.lru_cache(maxsize=None)
def _q(D, dt, hq, lq, which):
    """``[nb, hq, lq, D]`` (HND)."""
    g = torch.Generator().manual_seed(73 + D + 7 * hq + lq)
    return torch.randn(len(TABLES[which][0]), hq, lq, D, generator=g).to(dt).to(DEV)


def _starts(which):
    return _ints([s for _, s in TABLES[which][0]])


def _dense_calls():
    """(name, keywords, (causal, W)) of the calls of a dense route on the shared cache."""
    s = _starts("main")
    yield "non-causal", dict(), (False, 0)
    yield "offsets", dict(is_causal=True, q_start=s), (True, 0)
    for W in lp.paged_windows():
        yield f"offsets, window {W}", dict(is_causal=True, q_start=s, window_size=(W - 1, 0)), (True, W)


def _samples_differ(got, want, what, describe):
    """``_bits_equal`` per sample: the message names the samples that differ and the model's forms of their query blocks."""
    bits = lambda t: t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    nb = got[0].shape[0]
    bad = ((bits(got[0]) != bits(want[0])).view(nb, -1).sum(1) + (bits(got[1]) != bits(want[1])).view(nb, -1).sum(1)).tolist()
    names = [f"sample {b} ({n} elements) {describe(b)}" for b, n in enumerate(bad) if n]
    assert not names, f"{what}: {len(names)} samples differ: " + "; ".join(names[:6])


def _dense_describe(lq, causal, W):
    plans = lp.paged_plans(lq, causal, W)
    return lambda b: f"len {lp.PAGED_SAMPLES[b][0]} offset {lp.PAGED_SAMPLES[b][1]}: " + " ".join(lp.describe(plans[b, j]) for j in range(lp.nblk(lq)))


# ---------------------------------------------------------------------------------------------- the anchor
def _anchor_rows(oracle, tag, D, dt, cap, k_rows, v_rows, k_mean, v_amax, q_b, o_b, lse_b, causal, start, W):
    """One sample of a call -- q_b ``[Hq, Lq, D]``, o_b ``[Hq, Lq, D]``, lse_b ``[Hq, Lq]`` -- against the attention reference on the ledger's
    operands: the raw rows k_rows / v_rows ``[Hkv, L, D]`` the sample was given and its frozen statistics (k_mean ``[Hkv, D]`` or None, v_amax
    ``[Hkv, D]``), quantised by the oracle, at the bars of the random programs."""
    code, L = (0 if dt == F16 else 1), k_rows.shape[1]
    led = sim.Ledger(oracle, 1, k_rows.shape[0], D, code, cap)
    led.seed([0], None if k_mean is None else [util.bits(k_mean)], [v_amax.float().cpu().numpy()])
    led.append(0, util.bits(k_rows), util.bits(v_rows))
    ops = led.operands(0)
    Lq = q_b.shape[1]
    keep = rw.visible_from_keywords(Lq, L, (W - 1, 0) if W else (-1, -1), causal, start if causal else 0, L)
    assert bool(keep.any()), tag
    return check_sample_quantised(oracle, tag, util.bits(q_b), ops["K8"], ops["k_scale"], ops["V8"], ops["v_scale"], led.k_mean[0], code, D, keep,
                                  o_b.float().cpu().numpy(), lse_b.float().cpu().numpy())


def _anchor(oracle, tag, D, dt, which, b, q_b, o_b, lse_b, causal, start, W):
    """Sample ``b`` of a call on the shared cache of table ``which``."""
    k, v, km, v_amax, lens = _content(D, dt, which)
    L = int(lens[b])
    return _anchor_rows(oracle, tag, D, dt, TABLES[which][1], k[b, :, :L], v[b, :, :L], km[b], v_amax[b], q_b, o_b, lse_b, causal, start, W)


# ---------------------------------------------------------------------------------------------- f8p
@pytest.mark.parametrize("group", lp.PAGED_GROUPS, ids=[f"g{g}" for g in lp.PAGED_GROUPS])
@pytest.mark.parametrize("page_size", PAGES, ids=PAGE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_f8p_every_loop_form_is_the_contiguous_caches(oracle_mod, case, page_size, group):
    D, dt = case
    ref, c = _caches(D, dt, page_size, "main")
    q = _q(D, dt, HKV * group, lp.LQ, "main")
    for name, kw, (causal, W) in _dense_calls():
        want = sageattn_kvcache(q, ref, return_lse=True, **kw)
        got = sageattn_kvcache(q, c, return_lse=True, **kw)
        _samples_differ(got, want, f"f8p d{D} page {page_size} group {group} {name}", _dense_describe(lp.LQ, causal, W))
        if group == 4 and W and W == lp.paged_window_anchor()[0]:
            _, b, p = lp.paged_window_anchor()
            _anchor(oracle_mod, f"ANCHOR f8p d{D} page {page_size} {name} sample {b} {lp.describe(p)}", D, dt, "main", b, q[b], got[0][b], got[1][b],
                    True, lp.PAGED_SAMPLES[b][1], W)
    want = sageattn_kvcache(q, ref, return_lse=True, is_causal=True, causal_align="bottom_right")
    _bits_equal(sageattn_kvcache(q, c, return_lse=True, is_causal=True, causal_align="bottom_right"), want, "bottom-right")


# ---------------------------------------------------------------------------------------------- f8pg
@pytest.mark.parametrize("lq", lp.PACK_LQS, ids=[f"lq{n}" for n in lp.PACK_LQS])
@pytest.mark.parametrize("group", lp.PACK_GROUPS, ids=[f"g{g}" for g in lp.PACK_GROUPS])
@pytest.mark.parametrize("page_size", PAGES, ids=PAGE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_f8pg_every_loop_form_is_the_contiguous_caches(oracle_mod, case, page_size, group, lq):
    D, dt = case
    ref, c = _caches(D, dt, page_size, "main")
    q = _q(D, dt, HKV * group, lq, "main")
    for name, kw, (causal, W) in _dense_calls():
        want = sageattn_kvcache(q, ref, return_lse=True, pack_gqa=True, **kw)
        got = sageattn_kvcache(q, c, return_lse=True, pack_gqa=True, **kw)
        _samples_differ(got, want, f"f8pg d{D} page {page_size} group {group} lq {lq} {name}", _dense_describe(lq, causal, W))
        if group == 4 and lq == 16 and name == "offsets":
            b, p = lp.paged_anchor(lp.paged_plans(lq, True))
            _anchor(oracle_mod, f"ANCHOR f8pg d{D} page {page_size} {name} sample {b} {lp.describe(p)}", D, dt, "main", b, q[b], got[0][b], got[1][b],
                    True, lp.PAGED_SAMPLES[b][1], 0)


# ---------------------------------------------------------------------------------------------- f8pks
# (Lq, group, the forms: packed?)
SPLIT_FORMS = ((1, 4, (True,)), (16, 5, (True, False)), (128, 4, (False,)))


def _split_describe(causal, lq, S):
    samples = lp.paged_split_samples()

    def describe(b):
        n, s = samples[b]
        plans = [lp.split_chunk(causal, lq, lp.LKP_SPLIT, n, s if causal else None, S, c) for c in range(S)]
        return f"len {n} offset {s}: " + " ".join(f"c{c}{lp.describe(p)}" for c, p in enumerate(plans) if p.lk and p.n_iters)
    return describe


@pytest.mark.parametrize("page_size", PAGES, ids=PAGE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_f8pks_every_loop_form_of_a_chunk_is_the_contiguous_splits(oracle_mod, case, page_size):
    D, dt = case
    ref, c = _caches(D, dt, page_size, "split")
    s = _starts("split")
    for lq, group, forms in SPLIT_FORMS:
        q = _q(D, dt, HKV * group, lq, "split")
        for causal, kw in ((False, dict()), (True, dict(is_causal=True, q_start=s))):
            for S in lp.PAGED_SPLITS:
                for pk in forms:
                    want = sageattn_kvcache(q, ref, num_splits=S, pack_gqa=pk, return_lse=True, **kw)
                    got = sageattn_kvcache_split(q, c, S, pack_gqa=pk, return_lse=True, **kw)
                    what = f"f8pks d{D} page {page_size} lq {lq} {'causal' if causal else 'nc'} S {S} {'packed' if pk else 'unpacked'}"
                    _samples_differ(got, want, what, _split_describe(causal, lq, S))
                    if lq == 16 and pk and causal and S == 2:
                        plans = lp.paged_split_plans(True, lq, S)
                        b, p = lp.paged_anchor(plans, key=lambda kk: kk[1] == 1 and plans[kk[0], 0].n_iters > 0)       # chunk 1, behind a chunk 0 with work
                        _anchor(oracle_mod, f"ANCHOR {what} sample {b} chunk 1 {lp.describe(p)}", D, dt, "split", b, q[b], got[0][b], got[1][b],
                                True, lp.paged_split_samples()[b][1], 0)


def _c_split(entry, q, cache, causal, starts, S, ws, gqa_pack):
    """``sage_kvpsplit_attn`` / ``sage_attn_fused_q_pv_f8_kvlens`` with a workspace of the test's own (tests/test_gpu_paged_split.py::_c_call)."""
    nb, hq, lq, D = q.shape
    o = torch.empty_like(q)
    lse = torch.empty((nb, hq, lq), dtype=torch.float32, device=DEV)
    attr = _cabi.launch_attr(ws, q_start=starts, kv_split=S, gqa_pack=gqa_pack)
    _, _, _, _, q_sb, q_sh, q_sl = sq._dims(q, "HND")
    _, _, _, _, k_sb, k_sh, k_sl = sq._dims(cache.k_int8, "HND")
    _, _, _, _, o_sb, o_sh, o_sl = sq._dims(o, "HND")
    code = 0 if q.dtype == F16 else 1
    tail = (q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, o_sb, o_sh, o_sl, int(causal), sc._sm_log2(D ** -0.5), code, code, sq._stream(q), _cabi.attr_arg(attr))
    if entry == "paged":
        rc = _cabi_kvpsplit.load().sage_kvpsplit_attn(
            sq._p(q), sq._p(cache.k_int8), sq._p(cache.v_image), sq._p(o), sq._p(lse), sq._p(cache.k_scale), sq._p(cache.v_scale), sq._p(cache.lens),
            sq._p(cache.block_table), cache.block_table.stride(0), cache.num_pages, cache.page_size, cache.max_pages_per_seq,
            nb, hq, cache.Hkv, lq, D, *tail)
        _cabi.check(rc, "sage_kvpsplit_attn")
    else:
        rc = _cabi.load().sage_attn_fused_q_pv_f8_kvlens(
            sq._p(q), sq._p(cache.k_int8), sq._p(cache.v_image), sq._p(o), sq._p(lse), sq._p(cache.k_scale), sq._p(cache.v_scale), None, sq._p(cache.lens),
            nb, hq, cache.Hkv, lq, cache.capacity, D, *tail)
        _cabi.check(rc, "sage_attn_fused_q_pv_f8_kvlens")
    torch.cuda.synchronize()
    return o, lse


@pytest.mark.parametrize("shape", [(128, BF16, 256, 16, 5, True, True, 3), (64, F16, 64, 128, 4, False, False, 2), (128, F16, 64, 1, 4, True, True, 5),
                                   (64, BF16, 256, 16, 5, False, True, 3)], ids=["d128-page256-lq16-s3", "d64-page64-lq128-s2", "d128-page64-lq1-s5", "d64-page256-lq16-s3"])
def test_f8pks_the_workspace_is_the_contiguous_splits_byte_for_byte(shape):
    D, dt, page_size, lq, group, causal, packed, S = shape
    ref, c = _caches(D, dt, page_size, "split")
    q = _q(D, dt, HKV * group, lq, "split")
    starts = _starts("split") if causal else None
    nbytes = _cabi.kv_split_ws_bytes(q.shape[0], HKV * group, lq, D, S)
    out = {}
    for entry, cache in (("paged", c), ("contiguous", ref)):
        ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV).view(torch.float32)
        out[entry] = _c_split(entry, q, cache, causal, starts, S, ws, packed) + (ws,)
    _bits_equal(out["paged"][:2], out["contiguous"][:2], "the C entries")
    a, b = _u8(out["paged"][2]), _u8(out["contiguous"][2])
    assert torch.equal(a, b), f"the split workspace differs in {int((a != b).sum())} of {a.numel()} bytes, first at byte {int((a != b).nonzero()[0])}"
    assert bool((a != 0xA5).any())


# ---------------------------------------------------------------------------------------------- f8pr, f8pb, f8pbg
def _ragged_calls():
    """(name, rotation, W, bottom-right?) of the calls of the ragged and step sweeps."""
    for r in range(lp.PAGED_ROTATIONS):
        yield f"rotation {r}", r, 0, False
    yield "rotation 2, bottom-right", 2, 0, True
    for i, W in enumerate(lp.paged_windows()):
        yield f"rotation {i % lp.PAGED_ROTATIONS}, window {W}", i % lp.PAGED_ROTATIONS, W, False


def _cu(counts):
    out = [0]
    for n in counts:
        out.append(out[-1] + n)
    return out


@functools.lru_cache(maxsize=None)
def _rows(D, dt, hq):
    """``[nb, MAX_ROWS, hq, D]`` (NHD): the rows a sequence takes its first Lq_b from, so that a packed call and the dense call of every
    sequence of one row count read the same tensor."""
    g = torch.Generator().manual_seed(79 + D + hq)
    return torch.randn(len(lp.PAGED_SAMPLES), MAX_ROWS, hq, D, generator=g).to(dt).to(DEV)


def _ragged_operands(D, dt, hq, rotation, W, bottom_right, slack=0):
    counts = lp.paged_ragged_counts(rotation)
    rows = _rows(D, dt, hq)
    q = torch.cat([rows[b, :n] for b, n in enumerate(counts)] + [rows[0, :slack]])
    kw = dict() if bottom_right else dict(q_start=_ints([max(s, -n) for (_, s), n in zip(lp.PAGED_SAMPLES, counts)]))
    if W:
        kw["window_size"] = (W - 1, 0)
    return counts, q, kw


@pytest.mark.parametrize("group", lp.PAGED_GROUPS, ids=[f"g{g}" for g in lp.PAGED_GROUPS])
@pytest.mark.parametrize("page_size", PAGES, ids=PAGE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_f8pr_every_sequence_is_the_dense_paged_call_of_its_rows(oracle_mod, case, page_size, group):
    D, dt = case
    hq = HKV * group
    _, smoothed = _caches(D, dt, page_size, "main")
    # The kernels' own LSE is compared: the same cache without its ``k_mean``, which at attention time feeds nothing but the q . k_mean term the
    # Python entry adds to the returned lse.  That term is a torch matmul in the input dtype, of [total, Hq, 1, D] rows here and of [B, Hq, L, D]
    # there, and its fp16 rounding is the BLAS kernel's of that shape: with it, 1 of 58048 lse values of the calls of rotation 3 at d64 fp16,
    # group 4 (sample 37, Lq 1; with and without a window, on either page size) differs between the routes, and none of any other call.  tests/test_gpu_kv_varlen.py holds the term at its shapes;
    # the count of each call is printed below.
    c = copy.copy(smoothed)
    c.k_mean = None
    bits = lambda t: t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)
    for name, rotation, W, bottom_right in _ragged_calls():
        counts, q, kw = _ragged_operands(D, dt, hq, rotation, W, bottom_right)
        cu = _cu(counts)
        o, lse = sageattn_kvcache_varlen(q, c, _ints(cu), MAX_ROWS, return_lse=True, **kw)
        assert o.shape == q.shape and lse.shape == (hq, cu[-1])
        o_s, lse_s = sageattn_kvcache_varlen(q, smoothed, _ints(cu), MAX_ROWS, return_lse=True, **kw)
        assert torch.equal(bits(o_s), bits(o)), f"{name}: o depends on k_mean"
        term_differs = 0
        plans = lp.paged_ragged_plans(rotation, W, bottom_right)
        bad = []
        for L in lp.PAGED_RAGGED_LQS:
            dkw = dict(kw, is_causal=True, tensor_layout="NHD", return_lse=True, **(dict(causal_align="bottom_right") if bottom_right else {}))
            od, ld = sageattn_kvcache(_rows(D, dt, hq)[:, :L].contiguous(), c, **dkw)
            idx = [b for b, n in enumerate(counts) if n == L]
            ld_s = sageattn_kvcache(_rows(D, dt, hq)[:, :L].contiguous(), smoothed, **dkw)[1]
            term_differs += sum(int((bits(lse_s[:, cu[b]:cu[b] + L]) != bits(ld_s[b])).sum()) for b in idx)
            ro = torch.stack([o[cu[b]:cu[b] + L] for b in idx])                        # [n, L, hq, D]
            rl = torch.stack([lse[:, cu[b]:cu[b] + L] for b in idx])                   # [n, hq, L]
            sel = torch.tensor(idx, device=DEV)
            n_bad = ((bits(ro) != bits(od[sel])).view(len(idx), -1).sum(1) + (bits(rl) != bits(ld[sel])).view(len(idx), -1).sum(1)).tolist()
            bad += [f"sample {b} Lq {L} ({n} elements) len {lp.PAGED_SAMPLES[b][0]} offset {lp.PAGED_SAMPLES[b][1]}: " +
                    " ".join(f"{plans[b, j][0]}{lp.describe(plans[b, j][1])}" for j in range(lp.nblk(L))) for b, n in zip(idx, n_bad) if n]
        print(f"f8pr d{D} page {page_size} group {group} {name}: with the q . k_mean term {term_differs} of {lse.numel()} lse values differ from the dense calls'")
        assert not bad, f"f8pr d{D} page {page_size} group {group} {name}: {len(bad)} sequences differ from their dense calls: " + "; ".join(bad[:6])
        ar, b, p = lp.paged_ragged_anchor("two0")
        if group == 4 and name == f"rotation {ar}":
            n = counts[b]
            _anchor(oracle_mod, f"ANCHOR f8pr d{D} page {page_size} {name} sample {b} Lq {n} {lp.describe(p)}", D, dt, "main", b,      # (the smoothed cache's lse)
                    q[cu[b]:cu[b] + n].transpose(0, 1), o_s[cu[b]:cu[b] + n].transpose(0, 1), lse_s[:, cu[b]:cu[b] + n], True, max(lp.PAGED_SAMPLES[b][1], -n), 0)


@pytest.mark.parametrize("group", lp.PACK_GROUPS, ids=[f"g{g}" for g in lp.PACK_GROUPS])
@pytest.mark.parametrize("page_size", PAGES, ids=PAGE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_f8pb_f8pbg_every_row_of_the_step_call_is_the_ragged_routes(oracle_mod, case, page_size, group):
    D, dt = case
    hq = HKV * group
    _, c = _caches(D, dt, page_size, "main")
    for name, rotation, W, bottom_right in _ragged_calls():
        counts, q, kw = _ragged_operands(D, dt, hq, rotation, W, bottom_right, slack=3)
        _assert_same(q, c, counts, MAX_ROWS, f"step d{D} page {page_size} group {group} {name}", **kw)
        for unit, band in (("f8pbg", "decode"), ("f8pb", "chunk")):
            ar, b, p = lp.paged_ragged_anchor(band)
            if group == 4 and name == f"rotation {ar}":
                cu, n = _cu(counts), counts[b]
                o, lse = sageattn_kvcache_step(q, c, _ints(cu), MAX_ROWS, return_lse=True, **kw)
                _anchor(oracle_mod, f"ANCHOR {unit} d{D} page {page_size} {name} sample {b} Lq {n} {lp.describe(p)}", D, dt, "main", b,
                        q[cu[b]:cu[b] + n].transpose(0, 1), o[cu[b]:cu[b] + n].transpose(0, 1), lse[:, cu[b]:cu[b] + n], True, max(lp.PAGED_SAMPLES[b][1], -n), 0)
