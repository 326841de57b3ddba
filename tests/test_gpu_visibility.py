"""GPU: WHICH KEYS each row attended to, read exactly through probe values of V (tests/ref_probe.py), on every attention route.

Every other GPU file holds a route to a reference, or to another route, through a tolerance on outputs that average hundreds of keys.  Here
channel ``d`` of V holds a single 1.0, in the row of key ``j0 + d``: ``o[i, d]`` is the weight of row ``i`` on that key, ``+0`` iff the key
is invisible.  A sweep over ``j0`` reads the whole visibility matrix as booleans; the signature holes (channels that must stay ``+0``, a
different set for every (sample, kv-head) of a call) catch V read from another sample, kv-head, sequence, page or slot; V rows behind a
sample's length carry the probe on, so a key read from there shows as well.  tests/test_probe_host.py pins the instrument on the
references and shows that five subtly wrong references are reported.

Assertions, per sample and sweep (``ref_probe.judge``): (1) the visibility read back equals the predicate for every query head, row and key,
no violation, ``lse = -inf`` exactly in the rows that see nothing; (2) each non-empty row's weights sum to 1 within the bar; (3) every
visible weight is within ``bar * w_ref`` plus one output ulp of ``w_ref``, the FP64 softmax of the scores of the oracle's quantised
operands.  ``bar = 2^-4 + 2^-8 + 2^-10`` on the FP8-PV routes (P to e4m3, output rounding, fp32 exp2 and sums), ``2^-11 + 2^-8 + 2^-10`` on
the FP16-PV routes: derived from the formats, not tuned.  Conditions, asserted on the reference before a kernel runs: the visible scores
of a row spread over at most 6 log2 units (every visible P a normal e4m3 number), every visible ``w_ref >= 2^-12``.

Operands: ``q = 0.5 randn``, ``k = randn + a per-channel offset``, one seed per sample (``ref_probe.SEEDS``); dense shapes Hq 4, Hkv 2,
Lq 200, Lk 320; (D, dtype, layout) in (64, fp16, HND), (128, bf16, NHD), (96, fp16, HND); six samples per call from the (len, q_start, W)
triples ``ref_probe.TRIPLES``.  ``num_splits`` does not combine with a bounded window: there the chunk boundaries (keys 192; 128 and 256;
every 64) fall inside the samples' visible key ranges, and the samples of 130, 64 and 0 keys leave chunks empty.

Measured on an MI355X -- per route the largest ``err / (bar * w_ref)`` of any case (each test prints its own) and the largest score
spread of its cases in log2 units.  No route failed the set equality or a bar.

    route                                                      ratio   spread
    fp8 plain, Lk 320 / 257                                    0.930   5.74
    fp8 kv_lens, full / causal                                 0.928   5.74
    fp8 q_start / causal_align="bottom_right"                  0.923   5.66
    fp8 window_size causal, W 65 / 64 / 37 / 50 / 1            0.928   5.49      (W 1: every weight exactly 1)
    fp8 window_size (100, 30) / (-1, 30), non-causal           0.922   5.72
    fp8 per_warp, two-level / single-level                     0.926   5.75
    fp8 per_thread, single-level / "fp32+fp32"                 0.928   5.74
    fp8 pack_gqa, Lq 1 / 17, without / with a window           0.927   5.74
    fp8 num_splits 2 / 3 / 5 / "auto"                          0.931   5.56
    fp8 varlen top-left / bottom-right / window 37             0.923   5.46
    cache contiguous / paged 64, 128 / forked 64, 128          0.928   5.74
    fp16 cuda / triton / varlen, fp16 outputs                  0.175   5.68
    fp16 cuda / triton / varlen, bf16 outputs                  0.802   5.75      (bf16's half ulp, 2^-9, over the bar)
    fp16 triton with a bool attn_mask                          0.165   5.16

The FP8-PV ratios are e4m3's half ulp over the bar: the restatement itself reads 0.88 - 0.92 on the CPU (tests/test_probe_host.py).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_probe as rp
import util

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention_amd as sa
    from sageattention_amd import _cabi, quant as sq
    from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
    from sageattention_amd.paged_kv_cache import PagedQuantizedKVCache
    DEV = torch.device("cuda:0")

F16, BF16 = torch.float16, torch.bfloat16
HKV, LQ, LK = rp.HKV, rp.LQ, rp.LK
CASES, IDS = list(rp.CASES), list(rp.CASE_IDS)
FP8 = lambda *a, **kw: sa.sageattn_qk_int8_pv_fp8_cuda(*a, **kw)
WIN = [rp.TRIPLES[t] for t in rp.BATCH_WINDOWS]              # (len, q_start, _) of the windowed calls


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _code(dt):
    return 0 if dt == F16 else 1


def _lay(t, layout):
    return t if layout == "HND" else t.transpose(1, 2).contiguous()


def _host(o, layout):
    """A device output in ``layout`` as float32 numpy, HND."""
    return (o if layout == "HND" else o.transpose(1, 2)).float().cpu().numpy()


def _ints(values, dtype=torch.int32):
    return torch.tensor(list(values), dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def _qk(D, dt, Hq=rp.HQ, Lq=LQ):
    """q [6, Hq, Lq, D], k [6, HKV, LK, D] on the host, HND: made once per case, never modified."""
    return rp.operands(D, dt, Hq, Lq)


@functools.lru_cache(maxsize=None)
def _aux(oracle, D, dt, Hq, Lq, bq, bk, n, kind="f8", km_n=None, rows=None):
    """The oracle's quantised operands of q[bq] (its first ``rows`` rows) against the first ``n`` keys of k[bk], K smoothed by the mean the
    GPU forms over the first ``km_n`` (default n) keys.  ``kind``: "f8" (per-thread, the FP8 default), "f8-warp", "f16", "f16_triton"."""
    q, k = _qk(D, dt, Hq, Lq)
    qb = q[bq:bq + 1, :, :rows].contiguous()
    kb = k[bk:bk + 1, :, :n].contiguous()
    kmk = k[bk:bk + 1, :, :km_n or n].contiguous().to(DEV)
    km = util.bits(sq.channel_mean(kmk if D in (64, 128) else F.pad(kmk, (0, 128 - D))))
    kw = dict(f8=dict(pv="f8", qk_quant_gran="per_thread", fp8_scores="exact"), f16=dict(pv="f16", qk_quant_gran="per_thread"),
              f16_triton=dict(pv="f16_triton"))
    kw["f8-warp"] = dict(pv="f8", qk_quant_gran="per_warp", fp8_scores="exact")
    _, _, aux = oracle.sageattn_dense(util.bits(qb), util.bits(kb), util.bits(torch.zeros_like(kb)), _code(dt), is_causal=False, km=km, **kw[kind])
    return aux


def _probe(route, D, dt, Hkv, masks, call, bar, n_sweep=LK, sig_of=None):
    """The engine.  ``masks``: name -> per sample ``(n, keep [Lq_b, n], aux or None)``; ``call(v)`` takes the probe ``v`` ``[B, Hkv, n_sweep,
    D]`` (host, HND; sample b's rows carry its probe on behind its length) and returns name -> ``(o per sample [Hq, Lq_b, D] float32, lse
    per sample or None)``.  ``sig_of[b]``: the sample whose signature sample b's V carries (default b).  Conditions first, then the
    sweeps, then ``ref_probe.judge`` on every sample of every mask.  Prints and returns (largest weight-error ratio, largest spread)."""
    B = len(next(iter(masks.values())))
    sig_of = list(range(B)) if sig_of is None else sig_of
    refs, spread = {}, 0.0
    for name, samples in masks.items():                                          # the conditions, on the reference alone
        for b, (n, keep, aux) in enumerate(samples):
            assert keep.shape[1] == n
            if n == 0 or not keep.any():
                refs[name, b] = np.zeros((aux["q8"].shape[1] if aux is not None else 0, keep.shape[0], n))
                continue
            w, s = rp.weights_fp64(aux, keep), rp.score_spread(aux, keep)
            rp.check_conditions(w, keep, s)
            refs[name, b], spread = w, max(spread, s)
    reads = {}                                                                   # (name, b, signature) -> ([(j0, o)], lse)
    for j0, sig in rp.sweeps(D, n_sweep, B, Hkv):
        v = torch.stack([rp.probe_v(Hkv, n_sweep, D, j0, sig[sig_of[b]], dt) for b in range(B)])
        for name, (os_, lses) in call(v).items():
            for b in range(B):
                entry = reads.setdefault((name, b, tuple(sig[sig_of[b]])), ([], []))
                entry[0].append((j0, os_[b]))
                entry[1].append(None if lses is None else lses[b])
    torch.cuda.synchronize()
    worst, known_any = 0.0, {}
    for (name, b, sig), (outs, lses) in reads.items():
        n, keep, _ = masks[name][b]
        w = refs[name, b]
        if w.shape[0] == 0:
            w = np.zeros((outs[0][1].shape[0],) + keep.shape)
        for lse in lses[1:]:                                                     # (the LSE does not depend on V)
            assert lse is None or np.array_equal(lse, lses[0], equal_nan=True), f"{route} {name} sample {b}: lse differs between probe calls"
        seen, known, weights, bad = rp.read_visibility(outs, n, list(sig), Hkv)
        worst = max(worst, rp.judge(seen, known, weights, bad, keep, w, bar, _code(dt), lse=lses[0], what=f"{route} {name} sample {b} sig {list(sig)}"))
        known_any[name, b] = known_any.get((name, b), False) | known
    for key, known in known_any.items():
        assert np.all(known), f"{route} {key}: {int((~known).sum())} keys never read"
    print(f"PROBE {route}: largest err / (bar w_ref) = {worst:.3f}, largest spread {spread:.2f} log2 units")
    return worst, spread


def _dense_masks(oracle, D, dt, samples, kind="f8", Hq=rp.HQ, Lq=LQ):
    """Per-sample ``(n, keep, aux)`` of a dense call on the first samples of the case's batch; ``samples``: ``(len, s, W, r, causal)``."""
    out = []
    for b, (n, s, W, r, causal) in enumerate(samples):
        n = max(0, min(n, LK))
        keep = rp.visible(Lq, n, s, W, r, causal)
        out.append((n, keep, _aux(oracle, D, dt, Hq, Lq, b, b, n, kind) if n else None))
    return out


def _dense_call(fn, D, dt, layout, B, kw, Hq=rp.HQ, Lq=LQ, n_keys=LK):
    """``call`` of the engine for a dense entry point: one mask, named "o"."""
    q, k = _qk(D, dt, Hq, Lq)
    qd, kd = _lay(q[:B].to(DEV), layout), _lay(k[:B, :, :n_keys].contiguous().to(DEV), layout)

    def call(v):
        out = fn(qd, kd, _lay(v[:, :, :n_keys].contiguous().to(DEV), layout), tensor_layout=layout, return_lse=True, **kw)
        return {"o": (_host(out[0], layout), out[1].cpu().numpy())}
    return call


# ---------------------------------------------------------------------------------------------- 1. sageattn_qk_int8_pv_fp8_cuda
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp8_plain(oracle_mod, case, causal):
    """The call without keywords, Lk 320 and a ragged 257 (top-left causal: key <= row)."""
    D, dt, layout = case
    for n in (LK, 257):
        masks = {"o": _dense_masks(oracle_mod, D, dt, [(n, 0, 0, 0, causal)] * 2)}
        _probe(f"fp8 plain Lk {n}", D, dt, HKV, masks, _dense_call(FP8, D, dt, layout, 2, dict(is_causal=causal), n_keys=n), rp.BAR_F8, n_sweep=n)


@pytest.mark.parametrize("name", ["kv_lens", "kv_lens-causal", "q_start", "bottom_right"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp8_lengths_and_offsets(oracle_mod, case, name):
    D, dt, layout = case
    samples = rp.dense_masks()[name]
    lens = _ints(s[0] for s in samples)
    kw = {"kv_lens": dict(is_causal=False), "kv_lens-causal": dict(is_causal=True),
          "q_start": dict(is_causal=True, q_start=_ints(s[1] for s in samples)),
          "bottom_right": dict(is_causal=True, causal_align="bottom_right")}[name]
    _probe(f"fp8 {name}", D, dt, HKV, {"o": _dense_masks(oracle_mod, D, dt, samples)}, _dense_call(FP8, D, dt, layout, 6, dict(kv_lens=lens, **kw)), rp.BAR_F8)


@pytest.mark.parametrize("W", rp.WINDOWS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp8_causal_window(oracle_mod, case, W):
    """``window_size=(W - 1, 0)`` is one window per call: every sample of the windowed batch is checked under each of the triples' windows."""
    D, dt, layout = case
    samples = rp.dense_masks()[f"window{W}"]
    kw = dict(is_causal=True, kv_lens=_ints(s[0] for s in samples), q_start=_ints(s[1] for s in samples), window_size=(W - 1, 0))
    _probe(f"fp8 window {W}", D, dt, HKV, {"o": _dense_masks(oracle_mod, D, dt, samples)}, _dense_call(FP8, D, dt, layout, 6, kw), rp.BAR_F8)


@pytest.mark.parametrize("ws", [(100, 30), (-1, 30)], ids=["100-30", "unbounded-30"])
@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_fp8_non_causal_window(oracle_mod, case, ws):
    D, dt, layout = case
    samples = rp.dense_masks()[f"window({ws[0]},{ws[1]})"]
    kw = dict(is_causal=False, kv_lens=_ints(s[0] for s in samples), q_start=_ints(s[1] for s in samples), window_size=ws)
    _probe(f"fp8 window {ws}", D, dt, HKV, {"o": _dense_masks(oracle_mod, D, dt, samples)}, _dense_call(FP8, D, dt, layout, 6, kw), rp.BAR_F8)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("variant", [("per_warp", "fp32+fp16"), ("per_warp", "fp32"), ("per_thread", "fp32"), ("per_thread", "fp32+fp32")],
                         ids=["warp-two_level", "warp-single", "thread-single", "thread-fp32fp32"])
def test_fp8_granularity_and_accumulation(oracle_mod, variant, causal):
    """``qk_quant_gran`` per_warp / per_thread and ``pv_accum_dtype`` two-level / single-level on the plain call, ragged Lk 257."""
    gran, accum = variant
    D, dt, layout = CASES[(gran == "per_warp") ^ (accum == "fp32")]
    masks = {"o": _dense_masks(oracle_mod, D, dt, [(257, 0, 0, 0, causal)] * 2, kind="f8" if gran == "per_thread" else "f8-warp")}
    kw = dict(is_causal=causal, qk_quant_gran=gran, pv_accum_dtype=accum)
    _probe(f"fp8 {gran} {accum}", D, dt, HKV, masks, _dense_call(FP8, D, dt, layout, 2, kw, n_keys=257), rp.BAR_F8, n_sweep=257)


# ---------------------------------------------------------------------------------------------- 2. pack_gqa, num_splits
DECODE_LENS = (320, 257, 193, 130, 1, 0)
SPLIT_LENS = (320, 257, 193, 130, 64, 0)


@pytest.mark.parametrize("W", [0, 50], ids=["nowindow", "window50"])
@pytest.mark.parametrize("lq", [1, 17])
@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_fp8_pack_gqa(oracle_mod, case, lq, W):
    """Hq 8 / Hkv 2: four query heads of a kv-head share a workgroup.  Bottom-right with kv_lens; the holes show that every packed query head
    read its own group's V."""
    D, dt, layout = case
    samples = [(n, n - lq, W, 0, True) for n in DECODE_LENS]
    kw = dict(is_causal=True, causal_align="bottom_right", kv_lens=_ints(DECODE_LENS), pack_gqa=True)
    if W:
        kw["window_size"] = (W - 1, 0)
    masks = {"o": _dense_masks(oracle_mod, D, dt, samples, Hq=8, Lq=lq)}
    _probe(f"fp8 pack_gqa Lq {lq}" + (" window" if W else ""), D, dt, HKV, masks, _dense_call(FP8, D, dt, layout, 6, kw, Hq=8, Lq=lq), rp.BAR_F8)


@pytest.mark.parametrize("S", [2, 3, 5, "auto"])
@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_fp8_num_splits(oracle_mod, case, S):
    """Lq 16, bottom-right with kv_lens: T = 3, 2, 1 tiles per chunk put the chunk boundaries at keys 192; 128 and 256; every 64 -- inside
    the visible keys of the longer samples -- and the samples of 130, 64 and 0 keys leave chunks empty.  The merge leaves exact zeros exact."""
    D, dt, layout = case
    samples = [(n, n - 16, 0, 0, True) for n in SPLIT_LENS]
    kw = dict(is_causal=True, causal_align="bottom_right", kv_lens=_ints(SPLIT_LENS), num_splits=S)
    masks = {"o": _dense_masks(oracle_mod, D, dt, samples, Lq=16)}
    _probe(f"fp8 num_splits {S}", D, dt, HKV, masks, _dense_call(FP8, D, dt, layout, 6, kw, Lq=16), rp.BAR_F8)


# ---------------------------------------------------------------------------------------------- 3. FP16-PV, dense
def _fp16_cuda(*a, **kw):
    return sa.sageattn_qk_int8_pv_fp16_cuda(*a, **kw)


def _fp16_triton(*a, **kw):
    return sa.sageattn_qk_int8_pv_fp16_triton(*a, **kw)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("route", ["cuda", "triton"])
@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_fp16_dense(oracle_mod, case, route, causal):
    """The FP16-PV entry points (P rounded to fp16: the narrow bar).  Causal: a square call of 200 rows and keys; full: 257 keys."""
    D, dt, layout = case
    n = LQ if causal else 257
    fn, kind = (_fp16_cuda, "f16") if route == "cuda" else (_fp16_triton, "f16_triton")
    masks = {"o": _dense_masks(oracle_mod, D, dt, [(n, 0, 0, 0, causal)] * 2, kind=kind)}
    _probe(f"fp16 {route}", D, dt, HKV, masks, _dense_call(fn, D, dt, layout, 2, dict(is_causal=causal), n_keys=n), rp.BAR_F16, n_sweep=n)


def test_fp16_triton_attn_mask(oracle_mod):
    """The triton-named call with a bool ``attn_mask`` holding a window predicate (64 keys ending 57 right of the row: no row is empty)."""
    D, dt, layout = CASES[0]
    keep = rp.visible(LQ, 257, 57, 64)
    mask = torch.from_numpy(keep).to(DEV)[None, None]
    masks = {"o": [(257, keep, _aux(oracle_mod, D, dt, rp.HQ, LQ, b, b, 257, "f16_triton")) for b in range(2)]}
    _probe("fp16 triton attn_mask", D, dt, HKV, masks, _dense_call(_fp16_triton, D, dt, layout, 2, dict(attn_mask=mask), n_keys=257), rp.BAR_F16,
           n_sweep=257)


# ---------------------------------------------------------------------------------------------- 4. packed batches
SEQS = ((70, 193), (40, 130), (5, 0), (100, 40))        # (Lq, Lk): Lq != Lk everywhere, one without keys, one with more rows than keys
VARLEN_SEEDS = {64: (3, 0, 0, 0), 128: (0, 0, 0, 0)}     # per sequence: the first seeds that meet the conditions with room, as ref_probe.SEEDS


@functools.lru_cache(maxsize=None)
def _packed(D, dt):
    """q [sum Lq, HQ, D], k [sum Lk, HKV, D] on the host and the prefix arrays."""
    parts = [rp.qk(1, rp.HQ, HKV, lq, lk, D, dt, seed) for (lq, lk), seed in zip(SEQS, VARLEN_SEEDS[D])]
    q = torch.cat([p[0][0].transpose(0, 1) for p in parts]).contiguous()
    k = torch.cat([p[1][0].transpose(0, 1) for p in parts]).contiguous()
    cu = lambda xs: torch.tensor(np.concatenate([[0], np.cumsum(xs)]), dtype=torch.int32)
    return q, k, cu([s[0] for s in SEQS]), cu([s[1] for s in SEQS])


@functools.lru_cache(maxsize=None)
def _packed_aux(oracle, D, dt):
    """Per sequence, the operands of the packed routes: per-block INT8 Q with ``sm_scale log2(e)`` folded in, K smoothed by the mean over
    ALL packed tokens, Triton rounding (``oracle.sageattn_varlen``'s own steps); ``c = 1``."""
    O, code = oracle, _code(dt)
    q, k, cu_q, cu_k = _packed(D, dt)
    kind = "f16" if code == 0 else "bf16"
    km = util.bits(sq.channel_mean_packed(k.to(DEV), cu_k.to(DEV), sq.varlen_plan(cu_q.to(DEV), cu_k.to(DEV), total_q=q.shape[0], total_k=k.shape[0])))
    ks = O.convert(O.to_f32(util.bits(k), code) - O.to_f32(km.reshape(1, HKV, D), code), kind)
    qb_, out = util.bits(q), []
    for b, (lq, lk) in enumerate(SEQS):
        if lk == 0:
            out.append(None)
            continue
        q0, k0 = int(cu_q[b]), int(cu_k[b])
        qb = np.ascontiguousarray(qb_[q0:q0 + lq].transpose(1, 0, 2))[None]
        kb = np.ascontiguousarray(ks[k0:k0 + lk].transpose(1, 0, 2))[None]
        gq, nq = O.group_index(lq, "per_block", "q", 128, 128)
        gk, nk = O.group_index(lk, "per_block", "k", 64, 64)
        q8, qsc = O.quant_int8(qb, code, gq, nq, pre_scale=np.float32(D ** -0.5 * O.LOG2E), style=O.STYLE_TRITON)
        k8, ksc = O.quant_int8(kb, code, gk, nk, style=O.STYLE_TRITON)
        out.append(dict(q8=q8, qs=qsc, k8=k8, ks=ksc, gq=gq, gk=gk, c=1.0))
    return out


def _packed_masks(oracle, D, dt, s_of, W, causal=True):
    """Per sequence ``(Lk, keep, aux)``: row i sees key j iff ``s_of(lq, lk) + i - W < j <= s_of(lq, lk) + i``."""
    aux = _packed_aux(oracle, D, dt)
    return [(lk, rp.visible(lq, lk, s_of(lq, lk), W, 0, causal), aux[b]) for b, (lq, lk) in enumerate(SEQS)]


def _packed_call(fn, D, dt, kw, with_lse):
    q, k, cu_q, cu_k = _packed(D, dt)
    qd, kd, cq, ck = q.to(DEV), k.to(DEV), cu_q.to(DEV), cu_k.to(DEV)
    mq, mk = max(s[0] for s in SEQS), max(s[1] for s in SEQS)

    def call(v):
        vp = torch.cat([v[b, :, :lk].transpose(0, 1) for b, (_, lk) in enumerate(SEQS)]).contiguous().to(DEV)
        out = fn(qd, kd, vp, cq, ck, mq, mk, **kw)
        o, lse = (out if with_lse else (out, None))
        o = o.float().cpu().numpy()
        os_ = [np.ascontiguousarray(o[int(cu_q[b]):int(cu_q[b + 1])].transpose(1, 0, 2)) for b in range(len(SEQS))]
        lses = None if lse is None else [lse.cpu().numpy()[:, int(cu_q[b]):int(cu_q[b + 1])] for b in range(len(SEQS))]
        return {"o": (os_, lses)}
    return call


PACKED_MASKS = {"top_left": (dict(is_causal=True), lambda lq, lk: 0, 0),
                "bottom_right": (dict(is_causal=True, causal_align="bottom_right"), lambda lq, lk: lk - lq, 0),
                "window37": (dict(is_causal=True, causal_align="bottom_right", window_size=(36, 0)), lambda lq, lk: lk - lq, 37)}


@pytest.mark.parametrize("name", list(PACKED_MASKS))
@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_fp8_varlen(oracle_mod, case, name):
    """Four packed sequences; the signatures are per (sequence, kv-head) and key positions count from the sequence's first key, so a key or a
    V row taken across a ``cu_seqlens`` boundary shows."""
    D, dt, _ = case
    kw, s_of, W = PACKED_MASKS[name]
    fn = lambda *a, **k_: sa.sageattn_qk_int8_pv_fp8_varlen(*a, return_lse=True, **k_)
    _probe(f"fp8 varlen {name}", D, dt, HKV, {"o": _packed_masks(oracle_mod, D, dt, s_of, W)}, _packed_call(fn, D, dt, kw, True), rp.BAR_F8,
           n_sweep=max(s[1] for s in SEQS))


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_fp16_varlen(oracle_mod, case, causal):
    D, dt, _ = case
    masks = {"o": _packed_masks(oracle_mod, D, dt, lambda lq, lk: 0, 0, causal)}
    _probe("fp16 varlen", D, dt, HKV, masks, _packed_call(sa.sageattn_varlen, D, dt, dict(is_causal=causal), False), rp.BAR_F16,
           n_sweep=max(s[1] for s in SEQS))


# ---------------------------------------------------------------------------------------------- 5. the KV caches
CACHE_SAMPLES = {"q_start": [(n, s, 0, 0, True) for n, s, _ in WIN], "window64": [(n, s, 64, 0, True) for n, s, _ in WIN],
                 "full": [(n, 0, 0, 0, False) for n, _, _ in WIN]}
CACHE_KW = {"q_start": dict(is_causal=True), "window64": dict(is_causal=True, window_size=(63, 0)), "full": dict(is_causal=False)}


def _fill(cache, k, v, lens, layout, first=150, have=None):
    """Append rows ``have .. lens[b]`` of k / v [B, HKV, LK, D] (device, HND) to the cache: one append of up to ``first`` rows, then
    single-row and 7-row appends in turn.  Every sample stands at ``min(p, lens[b])`` rows after the appends up to position p."""
    p = 0 if have is None else have
    end, step = max(lens), 0
    while p < end:
        T = min(first if step == 0 else (1, 7)[step & 1], LK - p)
        cache.append(_lay(k[:, :, p:p + T], layout), _lay(v[:, :, p:p + T], layout), _ints(max(0, min(n - p, T)) for n in lens), layout)
        p, step = p + T, step + 1


def _cache_call(cache_of, D, dt, layout, lens, names, starts):
    """``call`` of the engine: a fresh cache per probe (V enters through ``append``), then one ``sageattn_kvcache`` per mask name."""
    q, k = _qk(D, dt)
    qd, kd = _lay(q.to(DEV), layout), k.to(DEV)
    km = sq.channel_mean_kvlens(kd, _ints(lens))            # the statistics of the final content; v_amax seeded with ones, not from V

    def call(v):
        cache = cache_of()
        cache.seed(km, torch.ones(6, HKV, D, device=DEV))
        _fill(cache, kd, v.to(DEV), lens, layout)
        assert cache.lens.tolist() == list(lens)
        out = {}
        for name in names:
            kw = dict(CACHE_KW[name], q_start=_ints(starts)) if CACHE_KW[name]["is_causal"] else CACHE_KW[name]
            o, lse = sageattn_kvcache(qd, cache, layout, return_lse=True, **kw)
            out[name] = (_host(o, layout), lse.cpu().numpy())
        return out
    return call


@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_contiguous_cache(oracle_mod, case):
    """QuantizedKVCache filled by one append of 150 rows, then single-row and 7-row appends up to each sample's length; causal with q_start,
    with a window of 64, and non-causal on the same fill."""
    D, dt, layout = case
    lens, starts = [n for n, _, _ in WIN], [s for _, s, _ in WIN]
    masks = {name: _dense_masks(oracle_mod, D, dt, samples) for name, samples in CACHE_SAMPLES.items()}
    call = _cache_call(lambda: QuantizedKVCache.allocate(6, HKV, LK, D, dt, DEV), D, dt, layout, lens, list(masks), starts)
    _probe("cache contiguous", D, dt, HKV, masks, call, rp.BAR_F8)


def _paged(page_size, D, dt, B=6, seed=5):
    """A paged cache whose block table is a random choice from a pool of twice the pages the batch needs."""
    per_seq = (LK + page_size - 1) // page_size
    c = PagedQuantizedKVCache.allocate(2 * B * per_seq, page_size, B, per_seq, HKV, D, dt, DEV)
    perm = torch.randperm(2 * B * per_seq, generator=torch.Generator().manual_seed(seed))[:B * per_seq]
    c.block_table.copy_(perm.view(B, per_seq).to(torch.int32).to(DEV))
    return c


@pytest.mark.parametrize("page_size", [64, 128])
@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_paged_cache(oracle_mod, case, page_size):
    """The same fill and the same masks through a block table: each key's V row landed in, and is read from, its own page and slot."""
    D, dt, layout = case
    lens, starts = [n for n, _, _ in WIN], [s for _, s, _ in WIN]
    masks = {name: _dense_masks(oracle_mod, D, dt, samples) for name, samples in CACHE_SAMPLES.items()}
    call = _cache_call(lambda: _paged(page_size, D, dt), D, dt, layout, lens, list(masks), starts)
    _probe(f"cache paged {page_size}", D, dt, HKV, masks, call, rp.BAR_F8)


@pytest.mark.parametrize("page_size", [64, 128])
@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_paged_cache_fork(oracle_mod, case, page_size):
    """Slots 0 (257 keys) and 1 (193 keys) fork into slots 2 (the whole parent: its open page is copied) and 3 (``prefix_lens`` 150, which
    rounds down to 128); the children then append 20 and 30 rows of their own.  A child sees exactly its prefix's keys plus what it
    appended, the parents read after the children's appends as before them, bit for bit."""
    D, dt, layout = case
    q, k = _qk(D, dt)
    src = [0, 1, 0, 1]                                              # slot -> the sample whose q, k and signature it carries
    qd, kd = _lay(q[src].to(DEV), layout), k[src].to(DEV)
    parents, after = [257, 193, 0, 0], [257, 193, 277, 158]
    km = sq.channel_mean_kvlens(kd, _ints([257, 193, 257, 193]))   # the parents' frozen statistics: the children take them over

    def samples(lens, causal):
        return [(n, rp.visible(LQ, n, n - LQ, 0, 0, causal), _aux(oracle_mod, D, dt, rp.HQ, LQ, src[b], src[b], n, "f8", km_n=parents[b % 2]) if n else None)
                for b, n in enumerate(lens)]
    masks = {"before": samples(parents, True), "after": samples(after, True), "after-full": samples(after, False)}
    kw = dict(is_causal=True, causal_align="bottom_right")

    def call(v):
        vd = v.to(DEV)
        c = _paged(page_size, D, dt, B=4)
        c.seed(km, torch.ones(4, HKV, D, device=DEV))
        _fill(c, kd, vd, parents, layout)
        o0, lse0 = sageattn_kvcache(qd, c, layout, return_lse=True, **kw)
        spare = sorted(set(range(c.num_pages)) - set(c.block_table.flatten().tolist()))
        c.fork([0, 1], [2, 3], spare[:2], [257, 150])
        assert c.lens.tolist() == [257, 193, 257, 128]
        for slot, (p, T) in ((2, (257, 20)), (3, (128, 30))):          # the children's own rows, one child per append
            c.append(_lay(kd[:, :, p:p + T], layout), _lay(vd[:, :, p:p + T], layout), _ints(T if b == slot else 0 for b in range(4)), layout)
        assert c.lens.tolist() == after
        o1, lse1 = sageattn_kvcache(qd, c, layout, return_lse=True, **kw)
        o2, lse2 = sageattn_kvcache(qd, c, layout, return_lse=True, is_causal=False)
        assert torch.equal(o0[:2], o1[:2]) and torch.equal(lse0[:2], lse1[:2]), "a parent changed when its child appended"
        return {"before": (_host(o0, layout), lse0.cpu().numpy()), "after": (_host(o1, layout), lse1.cpu().numpy()),
                "after-full": (_host(o2, layout), lse2.cpu().numpy())}
    _probe(f"cache fork {page_size}", D, dt, HKV, masks, call, rp.BAR_F8, sig_of=src)
