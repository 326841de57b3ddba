"""GPU: per-sample query offsets (``q_start``) and bottom-right causal alignment (``causal_align``) of the dense FP8-PV entry point.

Row i of sample b attends to key j iff ``j <= q_start[b] + i`` and ``j < len_b``.  Two references:
  * an offset that is a multiple of 128 is, bit for bit, the plain causal call on the sample's valid keys with ``q_start`` junk rows in front
    of its queries (same query blocks, same Q groups, every work item the same tiles through the same bodies): ``torch.equal`` (with
    ``smooth_k`` the lse is compared where the kernel writes it: the entry point adds a torch matmul whose rounding depends on its shape);
  * any offset against the exact CPU oracle on the quantised operands of the unshifted sample, the shift restated by padding: zero rows in
    front of q8 for a positive offset, rows dropped for a negative one (they see nothing: o = 0, lse = -inf exactly).  The bar is the default
    routes' own, ``2e-3 max|ref| + one output ulp`` and LSE within 5e-3 (test_gpu_kv_lens.py::test_samples_vs_oracle).

Shapes are test_gpu_kv_lens.py's: B = 6, Hq = 4, Hkv = 2, Lk = 640, Lq = 200 (a half-empty second query block), D in {64, 128, 96}.  The
padding rows of k / v hold random data, so a kernel that attended to them would not pass.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util
from fence import FILLS, Fence

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sageattention as mirror
    import sageattention_amd as sa
    from sageattention_amd import _cabi, core, processors, quant as sq
    DEV = torch.device("cuda:0")

B, HQ, HKV, LK, LQ = 6, 4, 2, 640, 200
LENS = (640, 577, 200, 130, 64, 1)
ALIGNED = (0, 128, 256, 384)
# (length, offset): what each reaches is listed in DESIGN 3.10
PAIRS = ((640, 440), (640, 384), (577, 377), (130, -70), (200, 0), (64, 128), (1, 0), (0, 5), (640, 1000), (640, -1000))
F16, BF16 = torch.float16, torch.bfloat16
FP8 = lambda *a, **kw: sa.sageattn_qk_int8_pv_fp8_cuda(*a, **kw)

# (D, dtype, layout, smooth_k): every head dim x dtype, layouts and smooth_k alternating over them; the four (layout, smooth_k) pairs at D = 128
CASES = [(D, dt, ("HND", "NHD")[(i + j) & 1], bool(i & 1) != bool(j)) for i, D in enumerate((64, 128, 96)) for j, dt in enumerate((F16, BF16))]
CASES += [(128, F16, lay, sk) for lay in ("HND", "NHD") for sk in (False, True) if (128, F16, lay, sk) not in CASES]
IDS = [f"d{D}-{'f16' if dt == F16 else 'bf16'}-{lay}-{'sk' if sk else 'nosk'}" for D, dt, lay, sk in CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _cabi.load()


def _lay(t, layout):
    return t if layout == "HND" else t.transpose(1, 2).contiguous()


def _hnd(t, layout):
    return t if layout == "HND" else t.transpose(1, 2)


def _cut(t, b, n, layout):
    """Sample b's first n rows as a contiguous batch of one."""
    return (t[b:b + 1, :, :n] if layout == "HND" else t[b:b + 1, :n]).contiguous()


@functools.lru_cache(maxsize=None)
def _qkv(D, dt, layout, lq=LQ, seed=11):
    """q [B, HQ, lq, D], k / v [B, HKV, LK, D] in ``layout`` and 384 junk query rows: made once per case, never modified."""
    g = torch.Generator().manual_seed(seed + D + lq)
    q = torch.randn(B, HQ, lq, D, generator=g).to(dt)
    k = (torch.randn(B, HKV, LK, D, generator=g) + torch.randn(1, HKV, 1, D, generator=g)).to(dt)
    v = torch.randn(B, HKV, LK, D, generator=g).to(dt)
    junk = (3.0 * torch.randn(1, HQ, max(ALIGNED), D, generator=g)).to(dt)
    return tuple(_lay(t.to(DEV), layout) for t in (q, k, v, junk))


def _ints(values, dtype=torch.int32):
    return torch.tensor(list(values), dtype=dtype, device=DEV)


def _poisoned(t, lens, layout, byte):
    """``t`` with the rows from each sample's length on overwritten with ``byte``."""
    out = t.clone()
    raw = _hnd(out, layout).view(torch.int16)
    fill = int(np.array([byte, byte], dtype=np.uint8).view(np.int16)[0])
    for b, n in enumerate(lens):
        raw[b, :, max(0, min(n, LK)):] = fill
    return out


def _same(a, b, what=""):
    assert torch.equal(a[0], b[0]), f"{what}: o differs in {int((a[0] != b[0]).sum())} of {a[0].numel()} elements"
    assert torch.equal(a[1], b[1]), f"{what}: lse differs in {int((a[1] != b[1]).sum())} of {a[1].numel()} rows"


# ---------------------------------------------------------------------------------------------- 1. aligned offsets: the padded plain call
def _kernel_lse(q, k, v, layout, skip, kv_lens=None, q_start=None):
    """(o, lse) as the attention kernel writes them (log2 domain, no smooth_k correction) for a causal smooth_k call, rows ``skip:`` --
    the entry point's own steps: head-dim padding, its pre-pass (the length-aware sequence with ``kv_lens``), the fused-Q launch."""
    D = q.shape[-1]
    qp, kp, vp, _ = core._pad_head_dim(q, k, v)
    fused = False if kv_lens is not None else core._fused_prepass_wanted(kp, layout, None)
    _, _, k8, ks, vimg, vs, _ = core._prepass_kv(qp, kp, vp, layout, "per_thread", 64, True, False, False, fused, kv_lens=kv_lens)
    o, lse = core._attn_fused_q(core._aligned(qp, 8), k8, vimg, vs, ks, layout, True, core._sm_log2(D ** -0.5), True, kv_lens=kv_lens,
                                q_start=q_start)
    return (o[:, :, skip:] if layout == "HND" else o[:, skip:])[..., :D], lse[:, :, skip:]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_aligned_offsets_are_the_padded_plain_call(case):
    """(Without the feature the keyword does not exist; the attribute handed to the parent's library is ignored: the top-left result.)"""
    D, dt, layout, smooth_k = case
    q, k, v, junk = _qkv(D, dt, layout)
    kw = dict(tensor_layout=layout, is_causal=True, smooth_k=smooth_k, return_lse=True)
    cat = 2 if layout == "HND" else 1
    for s in ALIGNED:
        o, lse = FP8(q, k, v, kv_lens=_ints(LENS), q_start=_ints([s] * B), **kw)
        assert o.shape == q.shape and lse.shape == (B, HQ, LQ)
        raw = _kernel_lse(q, k, v, layout, 0, kv_lens=_ints(LENS), q_start=_ints([s] * B)) if smooth_k else None
        for b, n in enumerate(LENS):
            front = junk[:, :, :s] if layout == "HND" else junk[:, :s]
            op, lp = FP8(torch.cat((front, q[b:b + 1]), dim=cat), _cut(k, b, n, layout), _cut(v, b, n, layout), **kw)
            op = op[:, :, s:] if layout == "HND" else op[:, s:]
            what = f"offset {s}, sample {b} (len {n})"
            if not smooth_k:
                _same((o[b:b + 1], lse[b:b + 1]), (op, lp[:, :, s:]), what)
                continue
            # smooth_k: the entry point returns the kernel's lse / log2(e) + (q . km) * sm_scale, and q . km is a torch matmul rounded to the
            # input dtype whose last bit depends on the GEMM's shape (batch 6 x 200 rows here, batch 1 x 200 + s rows there).  So o is compared
            # through the entry point and the lse where the kernel writes it, with no matmul on either side: core._attn_fused_q on each side's
            # own pre-passed operands.  Both bit for bit.
            assert torch.equal(o[b:b + 1], op), f"{what}: o differs in {int((o[b:b + 1] != op).sum())} of {op.numel()} elements"
            _same((raw[0][b:b + 1], raw[1][b:b + 1]), _kernel_lse(torch.cat((front, q[b:b + 1]), dim=cat), _cut(k, b, n, layout),
                                                                 _cut(v, b, n, layout), layout, s), what + ", kernel outputs")
        assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all())


# ---------------------------------------------------------------------------------------------- 2. any offset: the exact CPU oracle
def _oracle_sample(oracle, qb, kb, vb, code, D, smooth_k, s):
    """Reference o (float32 [1, HQ, lq, D]) and lse of one sample at offset ``s`` (already clamped to [-lq, Lk]); qb / kb / vb: HND, on the
    device, kb / vb cut to the sample's length.  Rows that see nothing are exactly 0 / -inf."""
    lq, n = qb.shape[2], kb.shape[2]
    o_ref, lse_ref = np.zeros((1, HQ, lq, D), np.float32), np.full((1, HQ, lq), -np.inf, np.float32)
    drop = max(0, -s)
    if n == 0 or drop >= lq:
        return o_ref, lse_ref
    km = None
    if smooth_k:
        km = util.bits(sq.channel_mean(kb if D in (64, 128) else F.pad(kb, (0, 128 - D))))
    _, _, aux = oracle.sageattn_dense(util.bits(qb), util.bits(kb), util.bits(vb), code, is_causal=True, pv="f8", qk_quant_gran="per_thread",
                                      return_lse=True, km=km, smooth_k=smooth_k, fp8_scores="exact")
    q8, gq = aux["q8"], aux["gq"]
    front = max(0, s)
    q8s = np.ascontiguousarray(np.concatenate([np.zeros(q8.shape[:2] + (front, q8.shape[3]), np.int8), q8[:, :, drop:]], axis=2))
    gqs = np.concatenate([np.zeros(front, np.int32), gq[drop:]])
    o, lse = oracle.attn(q8s, aux["k8"], aux["v8"], aux["qs"], gqs, aux["ks"], aux["gk"], causal=True, c=aux["c"],
                         pv_mode=oracle.PV_F8_TWO_LEVEL, out_dtype=code, v_scale=aux["vs"], return_lse=True, score_mode=oracle.SCORES_EXACT)
    o_ref[:, :, drop:] = util.f32(o, code)[:, :, front:, :D]
    # sageattn_dense's own LSE post-processing (natural log; smooth_k: + q . km * sm_scale, the product rounded to the input dtype)
    lse = lse[:, :, front:] / np.float32(oracle.LOG2E)
    if smooth_k:
        kind = "f16" if code == 0 else "bf16"
        qf = oracle.to_f32(util.bits(qb if D in (64, 128) else F.pad(qb, (0, 128 - D))), code)
        kmf = np.repeat(oracle.to_f32(aux["km"], code), HQ // HKV, axis=1)
        corr = oracle.to_f32(oracle.convert(np.einsum("bhld,bhd->bhl", qf, kmf), kind), code)
        lse = lse + corr[:, :, drop:] * np.float32(1.0 / (D ** 0.5))
    lse_ref[:, :, drop:] = lse
    return o_ref, lse_ref


def _check_vs_oracle(oracle, case, q, k, v, lens, starts, o, lse):
    D, dt, layout, smooth_k = case
    code = 0 if dt == F16 else 1
    lq = _hnd(q, layout).shape[2]
    for b, (n, s) in enumerate(zip(lens, starts)):
        n_c, s_c = max(0, min(n, LK)), max(-lq, min(s, LK))
        qb, kb, vb = (_hnd(t, layout).contiguous() for t in (q[b:b + 1], _cut(k, b, n_c, layout), _cut(v, b, n_c, layout)))
        ref, lse_ref = _oracle_sample(oracle, qb, kb, vb, code, D, smooth_k, s_c)
        got, lgot = _hnd(o[b:b + 1], layout).float().cpu().numpy(), lse[b:b + 1].cpu().numpy()
        empty = np.isneginf(lse_ref)                      # rows with q_start + i < 0, or a sample without keys
        assert empty.sum() == HQ * (lq if n_c == 0 else min(lq, max(0, -s_c))), (b, n, s)
        scale = float(np.abs(ref).max())
        err = float(np.abs(got - ref).max())
        lerr = float(np.abs(lgot[~empty] - lse_ref[~empty]).max()) if (~empty).any() else 0.0
        print(f"sample {b} len {n} offset {s}: max|diff| {err:.3e} (bar {2e-3 * scale + util.out_ulp(scale, code):.3e}), lse {lerr:.3e}, "
              f"{int(empty.sum())} empty rows")
        assert np.isfinite(got).all() and not np.isnan(lgot).any(), (b, n, s)
        assert np.array_equal(np.isneginf(lgot), empty), (b, n, s)
        assert not got[empty].any() and not np.signbit(got[empty]).any(), (b, n, s)            # +0, not merely small
        assert err <= 2e-3 * scale + util.out_ulp(scale, code), (b, n, s)
        assert lerr <= 5e-3, (b, n, s)


@pytest.mark.parametrize("case", CASES[:6], ids=IDS[:6])
def test_any_offset_vs_oracle(oracle_mod, case):
    D, dt, layout, smooth_k = case
    q, k, v, _ = _qkv(D, dt, layout)
    kw = dict(tensor_layout=layout, is_causal=True, smooth_k=smooth_k, return_lse=True)
    for pairs in (PAIRS[:B], PAIRS[-B:]):
        lens, starts = [p[0] for p in pairs], [p[1] for p in pairs]
        o, lse = FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints(starts), **kw)
        _check_vs_oracle(oracle_mod, case, q, k, v, lens, starts, o, lse)


@pytest.mark.parametrize("lq", [1, 16])
@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_decode_shapes_vs_oracle(oracle_mod, case, lq):
    """Lq = 1 and 16 new rows at the end of each sample's keys (Lq = 16 against one key: fifteen rows in front of key 0)."""
    D, dt, layout, smooth_k = case
    q, k, v, _ = _qkv(D, dt, layout, lq=lq)
    kw = dict(tensor_layout=layout, is_causal=True, smooth_k=smooth_k, return_lse=True)
    o, lse = FP8(q, k, v, kv_lens=_ints(LENS), causal_align="bottom_right", **kw)
    _check_vs_oracle(oracle_mod, case, q, k, v, LENS, [n - lq for n in LENS], o, lse)


# ---------------------------------------------------------------------------------------------- 3. the keywords
def test_the_keywords_mean_what_they_say():
    case = CASES[1]
    D, dt, layout, smooth_k = case
    q, k, v, _ = _qkv(D, dt, layout)
    kw = dict(tensor_layout=layout, is_causal=True, smooth_k=smooth_k, return_lse=True)
    lens = (640, 577, 200, 130, 0, 900)
    clamped = [max(0, min(n, LK)) for n in lens]
    br = FP8(q, k, v, kv_lens=_ints(lens), causal_align="bottom_right", **kw)
    _same(br, FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints([n - LQ for n in clamped]), **kw), "bottom_right with kv_lens")
    assert not torch.equal(br[0], FP8(q, k, v, kv_lens=_ints(lens), **kw)[0])                       # (the alignment is not ignored)
    _same(FP8(q, k, v, causal_align="bottom_right", **kw), FP8(q, k, v, q_start=_ints([LK - LQ] * B), **kw), "bottom_right without kv_lens")
    _same(FP8(q, k, v, causal_align="bottom_right", **kw), FP8(q, k, v, kv_lens=_ints([LK] * B), q_start=LK - LQ, **kw), "full lengths")
    _same(FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints([0] * B), **kw), FP8(q, k, v, kv_lens=_ints(lens), **kw), "q_start = zeros")
    _same(FP8(q, k, v, q_start=0, **kw), FP8(q, k, v, **kw), "q_start = 0 without kv_lens: the plain causal call")
    # ... and on a ragged key range (577 keys: the plain pre-pass's zero-padded tail image under the KVLEN kernel)
    kr, vr = (t[:, :577].contiguous() if layout == "NHD" else t[:, :, :577].contiguous() for t in (k, v))
    _same(FP8(q, kr, vr, q_start=0, **kw), FP8(q, kr, vr, **kw), "q_start = 0 without kv_lens, Lk 577")
    _same(FP8(q, kr, vr, causal_align="bottom_right", **kw), FP8(q, k, v, kv_lens=_ints([577] * B), q_start=377, **kw), "bottom_right, Lk 577")
    starts = (440, 384, -3, 64, 5, 77)
    ref = FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints(starts), **kw)
    _same(FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints(starts, torch.int64), **kw), ref, "int64 offsets")
    _same(FP8(q, k, v, kv_lens=_ints(lens, torch.int64), q_start=_ints([2 ** 40 if s == 440 else s for s in starts], torch.int64), **kw),
          FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints([LK if s == 440 else s for s in starts]), **kw), "an int64 offset past int32")
    _same(FP8(q, k, v, kv_lens=_ints(lens), q_start=77, **kw), FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints([77] * B), **kw), "int offset")
    # sageattn forwards to the FP8 entry point with pv_accum_dtype="fp32+fp32" and smooth_k=True; processors.sdpa to sageattn
    for extra in (dict(q_start=_ints(starts)), dict(causal_align="bottom_right")):
        ref = FP8(q, k, v, kv_lens=_ints(lens), tensor_layout=layout, is_causal=True, return_lse=True, pv_accum_dtype="fp32+fp32", **extra)
        _same(sa.sageattn(q, k, v, tensor_layout=layout, is_causal=True, return_lse=True, kv_lens=_ints(lens), **extra), ref, "sageattn")
        _same(mirror.sageattn(q, k, v, tensor_layout=layout, is_causal=True, return_lse=True, kv_lens=_ints(lens), **extra), ref, "mirror")
        assert torch.equal(processors.sdpa(q, k, v, is_causal=True, tensor_layout=layout, kv_lens=_ints(lens), **extra), ref[0])
    ref = FP8(q, k, v, tensor_layout=layout, is_causal=True, pv_accum_dtype="fp32+fp32", causal_align="bottom_right")
    assert torch.equal(processors.sdpa(q, k, v, is_causal=True, tensor_layout=layout, causal_align="bottom_right"), ref)


# ---------------------------------------------------------------------------------------------- 4. the padding is never read
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5]], ids=[IDS[0], IDS[3], IDS[5]])
def test_padding_is_never_read(case):
    """Padding rows of k / v as NaN patterns (0xFF bytes) and 0x5A bytes: the bits of the run on random padding, finite where rows see keys --
    plainly, and inside the fenced, poisoned allocator, where no guard byte may change and the outputs lie inside their arenas."""
    D, dt, layout, smooth_k = case
    q, k, v, _ = _qkv(D, dt, layout)
    kw = dict(tensor_layout=layout, is_causal=True, smooth_k=smooth_k, return_lse=True)
    lens, starts = [p[0] for p in PAIRS[:B]], [p[1] for p in PAIRS[:B]]
    ref = FP8(q, k, v, kv_lens=_ints(lens), q_start=_ints(starts), **kw)
    sees = torch.isfinite(ref[1])
    assert int((~sees).sum()) == HQ * 70 and bool(torch.isneginf(ref[1][~sees]).all())            # (130, -70): seventy rows in front of key 0
    assert bool(torch.isfinite(ref[0].float()).all())
    for fill in FILLS:
        kp, vp = _poisoned(k, lens, layout, fill), _poisoned(v, lens, layout, fill)
        _same(FP8(q, kp, vp, kv_lens=_ints(lens), q_start=_ints(starts), **kw), ref, f"padding byte 0x{fill:02X}")
        with Fence(fill) as f:
            got = FP8(f.input(q), f.input(kp), f.input(vp), kv_lens=f.input(_ints(lens)), q_start=f.input(_ints(starts)), **kw)
            f.check()
            _same(got, ref, f"fill 0x{fill:02X}, fenced")
            if D in (64, 128):
                assert f.owns(got[0])
        with Fence(fill) as f:                                   # without kv_lens: the plain pre-pass, lengths filled with Lk
            full = FP8(f.input(q), f.input(k), f.input(v), q_start=f.input(_ints(starts)), **kw)
            f.check()
        _same(full, FP8(q, k, v, kv_lens=_ints([LK] * B), q_start=_ints(starts), **kw), f"fill 0x{fill:02X}, fenced, no kv_lens")


# ---------------------------------------------------------------------------------------------- 5. graph capture
def test_graph_capture_follows_both_tensors():
    """Captured once; each replay computes with what q_start and kv_lens hold then: no host read, no decision on the host."""
    D, dt, layout = 128, F16, "HND"
    q, k, v, _ = _qkv(D, dt, layout)
    kw = dict(tensor_layout=layout, is_causal=True, return_lse=True)
    first = (LENS, tuple(n - LQ for n in LENS))
    second = ((3, 640, 0, 129, 448, 65), (0, 384, 7, -100, 300, 64))
    lens, starts = _ints(first[0]), _ints(first[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        FP8(q, k, v, kv_lens=lens, q_start=starts, **kw)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o, lse = FP8(q, k, v, kv_lens=lens, q_start=starts, **kw)
    for n_values, s_values in (second, first):
        lens.copy_(_ints(n_values))
        starts.copy_(_ints(s_values))
        g.replay()
        eager = FP8(q, k, v, kv_lens=_ints(n_values), q_start=_ints(s_values), **kw)
        torch.cuda.synchronize()
        _same((o, lse), eager, f"replay with {n_values} / {s_values}")
