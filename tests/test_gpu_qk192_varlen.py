"""GPU: ``sageattention_amd.qk192_varlen.sageattn_qk192_varlen``, the packed variable-length form of the 192-wide Q / K, 128-wide V FP8-PV route.

1. Without a mask and top-left, every sequence's rows of ``o`` and ``lse`` equal bit for bit ``sageattn_qk192`` on the slice with B = 1 (which
   tests/test_gpu_qk192.py holds to the restatement and to FP64); a sequence without keys gives ``o = +0`` and ``lse = -inf``.
2. Bottom-right, against the CPU restatement assembled from tests/ref_fp8_torch.py per sequence and head: K at 192 channels against the
   sequence's own mean, V padded to 192, Q with its own groups, and ``attn_fp8(causal=True)`` with the diagonal moved by padding ``q8`` in front
   with ``Lk_s - Lq_s`` zero rows (slot 0) or dropping the first ``Lq_s - Lk_s`` rows: a wholly masked tile is an exact no-op there, so the padding
   moves the diagonal and nothing else.  Bars: tests/test_gpu_qk192.py::_hold (2e-3 max|o| + one output ulp; LSE 5e-3; against FP64 no worse than
   the restatement's own error plus that bar).  Rows in front of key 0: ``o == 0`` exactly, ``lse == -inf``.
3. A ``cu_seqlens_k`` whose last entry exceeds ``total_k``: the C calls return and nothing outside their own buffers is written.

Each list of ``(Lq_s, Lk_s)`` is the smallest that reaches one mechanism (see CASES)."""
import math

import pytest
import torch
import torch.nn.functional as F

import util  # noqa: F401  (sys.path)
import ref_fp8_torch as ref
from test_gpu_qk192 import _hold

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
# (sequences, Dqk, Dv, (Hq, Hkv), dtype, smooth_k, sm_scale)
CASES = [
    ([(1, 1)], 192, 128, (2, 2), F16, True, None),                                   # minimal call
    ([(33, 65), (128, 64), (1, 200)], 160, 72, (4, 2), BF16, True, None),            # partial wave, ragged tile, a decode-like row, a tile base that is not tokens / 64
    ([(129, 192), (0, 70), (257, 449)], 192, 128, (2, 2), F16, False, None),         # a sequence without rows, the ring wrapping, steady state
    ([(72, 200), (40, 0), (200, 72)], 136, 128, (4, 2), BF16, True, 0.07),           # a sequence without keys in the middle, more rows than keys
    ([(130, 450), (64, 64)], 192, 128, (2, 2), F16, True, None),                     # bottom-right shift that is no multiple of 32
    ([(33, 63), (33, 64), (33, 65)], 192, 128, (2, 2), BF16, True, None),            # the last key on either side of the first tile boundary ...
    ([(33, 127), (33, 128), (33, 129)], 192, 128, (4, 2), F16, True, None),          # ... and of the second
    ([(127, 192), (128, 192)], 192, 128, (2, 2), F16, True, None),                   # the last row on either side of the first block boundary ...
    ([(255, 192), (256, 192)], 160, 72, (4, 2), BF16, False, None),                  # ... and of the second
    ([(129, 65)], 192, 128, (8, 1), F16, True, None),                                # GQA groups of 8 and 4 at the smallest shape with two query blocks
    ([(129, 65), (130, 64)], 192, 128, (8, 2), BF16, True, None),
]
IDS = ["-".join(f"{a}x{b}" for a, b in c[0]) for c in CASES]


def _inputs(seqs, Dqk, Dv, heads, dtype):
    g = torch.Generator().manual_seed(sum(1000 * a + b for a, b in seqs) + Dqk + Dv)
    tq, tk = sum(a for a, _ in seqs), sum(b for _, b in seqs)
    q = torch.randn(tq, heads[0], Dqk, generator=g).to(dtype)
    k = (torch.randn(tk, heads[1], Dqk, generator=g) + 0.5).to(dtype)
    v = torch.randn(tk, heads[1], Dv, generator=g).to(dtype)
    cu = lambda ls: torch.tensor([0] + ls, dtype=torch.int64).cumsum(0).to(torch.int32)
    return q, k, v, cu([a for a, _ in seqs]), cu([b for _, b in seqs])


def _call(q, k, v, cu_q, cu_k, seqs, **kw):
    from sageattention_amd.qk192_varlen import sageattn_qk192_varlen
    dev = torch.device("cuda:0")
    o, lse = sageattn_qk192_varlen(q.to(dev), k.to(dev), v.to(dev), cu_q.to(dev), cu_k.to(dev), max(a for a, _ in seqs), max(b for _, b in seqs),
                                   return_lse=True, **kw)
    torch.cuda.synchronize()
    assert o.dtype == q.dtype and o.shape == q.shape[:2] + (v.shape[-1],) and lse.shape == (q.shape[1], q.shape[0]) and lse.dtype == torch.float32
    return o, lse


@pytest.mark.parametrize("causal", [False, True], ids=["none", "top_left"])
@pytest.mark.parametrize("seqs,Dqk,Dv,heads,dtype,smooth_k,sm_scale", CASES, ids=IDS)
def test_each_sequence_is_the_dense_call_bit_for_bit(seqs, Dqk, Dv, heads, dtype, smooth_k, sm_scale, causal):
    from sageattention_amd.qk192 import sageattn_qk192
    q, k, v, cu_q, cu_k = _inputs(seqs, Dqk, Dv, heads, dtype)
    o, lse = _call(q, k, v, cu_q, cu_k, seqs, is_causal=causal, causal_align="top_left", sm_scale=sm_scale, smooth_k=smooth_k)
    dev, equal = o.device, []
    for s, (lq, lk) in enumerate(seqs):
        rq, rk = slice(cu_q[s].item(), cu_q[s + 1].item()), slice(cu_k[s].item(), cu_k[s + 1].item())
        if lq == 0:
            continue
        if lk == 0:
            assert (o[rq] == 0).all() and not torch.signbit(o[rq].float()).any() and (lse[:, rq] == -math.inf).all()
            continue
        od, lsed = sageattn_qk192(q[rq][None].to(dev), k[rk][None].to(dev), v[rk][None].to(dev), tensor_layout="NHD", is_causal=causal,
                                  sm_scale=sm_scale, smooth_k=smooth_k, return_lse=True)
        print(f"sequence {s} ({lq}, {lk}): o differs in {(o[rq] != od[0]).sum().item()} elements, lse in {(lse[:, rq] != lsed[0]).sum().item()} "
              f"(max {(lse[:, rq] - lsed[0]).abs().nan_to_num(0.0).max().item():.2e})")
        equal.append(torch.equal(o[rq], od[0]) and torch.equal(lse[:, rq], lsed[0]))
    assert all(equal)


def _restate(q, k, v, sm, smooth_k):
    """One sequence, bottom-right: (o [Lq, Hq, Dv], natural-log lse [Lq, Hq]) of the restatement, FP64; rows in front of key 0 are 0 / -inf."""
    (Lq, Hq, _), (Lk, Hkv, Dv), d = q.shape, v.shape, k.shape[0] - q.shape[0]
    q, k, v = (F.pad(t, (0, 192 - t.shape[-1])) for t in (q, k, v))
    (gq, nq), (gk, nk) = ref.groups(Lq, "per_thread", "q"), ref.groups(Lk, "per_thread", "k")
    o, lse = torch.zeros(Lq, Hq, Dv, dtype=torch.float64), torch.full((Lq, Hq), -math.inf, dtype=torch.float64)
    for h in range(Hq):
        hk = h // (Hq // Hkv)
        km = k[:, hk].float().mean(dim=0).to(k.dtype) if smooth_k else None
        k8, ks = ref.quant_int8_per_thread(k[:, hk], gk, nk, mean=km)
        v8, vs, _ = ref.quant_v_fp8(v[:, hk], False)
        q8, qs = ref.quant_int8_per_thread(q[:, h], gq, nq)
        q8p = torch.cat([torch.zeros(d, 192, dtype=torch.int8), q8]) if d >= 0 else q8[-d:]
        slot = torch.cat([torch.zeros(d, dtype=gq.dtype), gq]) if d >= 0 else gq[-d:]
        oo, ll = ref.attn_fp8(q8p, k8, v8, qs, slot, ks, gk, vs, None, causal=True, sm_scale=sm, two_level=True, out_dtype=q.dtype)
        rows = slice(max(-d, 0), Lq)
        o[rows, h] = oo[max(d, 0):, :Dv].double()
        lse[rows, h] = ll[max(d, 0):].double() / ref.LOG2E
        if smooth_k:
            lse[rows, h] += (q[rows, h].double() * km.double()).sum(-1) * sm
    return o, lse


@pytest.mark.parametrize("seqs,Dqk,Dv,heads,dtype,smooth_k,sm_scale", CASES, ids=IDS)
def test_bottom_right_matches_the_restatement_and_fp64(seqs, Dqk, Dv, heads, dtype, smooth_k, sm_scale):
    q, k, v, cu_q, cu_k = _inputs(seqs, Dqk, Dv, heads, dtype)
    o, lse = _call(q, k, v, cu_q, cu_k, seqs, is_causal=True, sm_scale=sm_scale, smooth_k=smooth_k)      # (causal_align: the default)
    o, lse, sm = o.cpu(), lse.cpu().t(), Dqk ** -0.5 if sm_scale is None else sm_scale
    for s, (lq, lk) in enumerate(seqs):
        rq, rk = slice(cu_q[s].item(), cu_q[s + 1].item()), slice(cu_k[s].item(), cu_k[s + 1].item())
        unseen = min(max(lq - lk, 0), lq) if lk > 0 else lq
        front = slice(rq.start, rq.start + unseen)
        assert (o[front] == 0).all() and not torch.signbit(o[front].float()).any() and (lse[front] == -math.inf).all()
        if unseen == lq:
            continue
        ro, rlse = _restate(q[rq], k[rk], v[rk], sm, smooth_k)
        g = heads[0] // heads[1]
        sc = torch.einsum("ihd,jhd->hij", q[rq].double(), k[rk].double().repeat_interleave(g, dim=1)) * sm
        keep = torch.arange(lk)[None, :] <= torch.arange(lq)[:, None] + (lk - lq)
        sc = sc.masked_fill(~keep, -math.inf)[:, unseen:]
        truth = (torch.einsum("hij,jhd->ihd", torch.softmax(sc, dim=-1), v[rk].double().repeat_interleave(g, dim=1)), torch.logsumexp(sc, dim=-1).t())
        seen = slice(rq.start + unseen, rq.stop)
        _hold(o[seen].double(), lse[seen].double(), ro[unseen:], rlse[unseen:], truth, dtype)


def test_a_prefix_beyond_the_rows_drops_work_and_writes_nothing_outside():
    """cu_seqlens_k ends 300 rows past total_k.  The buffers of the two C calls lie inside one poisoned arena with guard bands between them: the
    calls return, the device stays healthy and every guard byte is intact."""
    from sageattention_amd import _cabi_qk192v
    from sageattention_amd.quant import _p, _stream
    lib, dev = _cabi_qk192v.load(), torch.device("cuda:0")
    seqs, H = [(100, 100), (60, 90)], 2
    q, k, v, cu_q, cu_k = _inputs(seqs, 192, 128, (H, H), F16)
    tq, tk, nseq = q.shape[0], k.shape[0], len(seqs)
    cu_k[-1] += 300
    q, k, v, cu_q, cu_k = (t.to(dev) for t in (q, k, v, cu_q, cu_k))
    tiles = (tk + 63) // 64 + nseq
    ws_bytes = lib.sage_qk192v_ws_bytes(nseq, H, tq, tk)
    sizes = dict(k_img=H * tiles * 12288, v_img=H * tiles * 8192, k_scale=H * tiles * 16, v_scale=nseq * H * 512, k_mean=nseq * H * 384, ws=ws_bytes,
                 o=tq * H * 256, lse=H * tq * 4)
    GUARD, off, at = 4096, 4096, {}
    for name, n in sizes.items():
        at[name] = off
        off += (n + 255) // 256 * 256 + GUARD
    arena = torch.full((off,), 0xA5, dtype=torch.uint8, device=dev)
    b = {name: arena[at[name]:at[name] + n] for name, n in sizes.items()}
    rc = lib.sage_qk192v_prepass(_p(k), _p(v), _p(cu_q), _p(cu_k), _p(b["k_img"]), _p(b["k_scale"]), _p(b["k_mean"]), _p(b["v_img"]), _p(b["v_scale"]),
                                 _p(b["ws"]), ws_bytes, nseq, tq, tk, H, H, 192, 128, k.stride(0), k.stride(1), v.stride(0), v.stride(1), 2, 1, 0, _stream(q))
    assert rc == 0, lib.sage_last_error()
    rc = lib.sage_qk192v_attn(_p(q), _p(cu_q), _p(cu_k), _p(b["k_img"]), _p(b["v_img"]), _p(b["k_scale"]), _p(b["v_scale"]), _p(b["ws"]), ws_bytes,
                              _p(b["o"]), _p(b["lse"]), nseq, tq, tk, H, H, 192, 128, q.stride(0), q.stride(1), H * 128, 128, 2, 192 ** -0.5, 0, _stream(q))
    assert rc == 0, lib.sage_last_error()
    torch.cuda.synchronize()
    inside = torch.zeros(off, dtype=torch.bool, device=dev)
    for name, n in sizes.items():
        inside[at[name]:at[name] + n] = True
    assert (arena[~inside] == 0xA5).all()
    # the first sequence's prefix entries are sound: its rows are the well-formed call's
    o = b["o"].view(torch.float16).view(tq, H, 128)
    cu_k[-1] -= 300
    want, _ = _call(q, k, v, cu_q, cu_k, seqs, is_causal=True)
    assert torch.equal(o[:100], want[:100])
