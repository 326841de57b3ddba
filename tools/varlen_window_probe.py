#!/usr/bin/env python3
"""What a sliding window costs and saves on the packed FP8-PV route, on the serving mix of tools/varlen_br_probe.py: whole calls and the
attention kernel alone, interleaved.

  packed        sageattn_qk_int8_pv_fp8_varlen(..., is_causal=True, causal_align="bottom_right")                      (no window)
  packed_wmax   ... window_size=(2**30 - 2, 0): W = 2**30 - 1 cuts no row -- the windowed kernels on the unwindowed work: the flag's cost
  packed_w4096 / _w1024 / _w256   ... window_size=(W - 1, 0)
  dense_w4096 / _w1024 / _w256    sageattn_qk_int8_pv_fp8_cuda(q_padded, k_padded, v_padded, is_causal=True, kv_lens=Lk_b,
                causal_align="bottom_right", window_size=(W - 1, 0)): the same batch padded to [B, H, max Lq, D] / [B, H, max Lk, D], every
                sequence's rows right-aligned in its padded q -- what a caller with local layers had before

Mix (GQA 32 / 8, D = 128, bf16): six chunks of 512 rows against 2048 ... 8192 cached keys, 64 decode rows (Lq = 1) against 1024 ... 8192 keys
(seeded), one full 2048-row prefill.  Next to the times: the (row, key) pairs the mask attends to and ps per pair, the 64-key tiles the
kernel's loop bounds give (restated here as in tests/ref_varlen_window.py::loop_bounds; x Hq) and how many of them are head tiles, and the
time per work item (kernel time x resident workgroups / items).

"call" is the whole entry point (plan + pre-pass + attention); "kernel" is the attention launch alone on operands prepared once.  Per round
every variant is warmed, then timed call by call with device events; the figure of a variant is the median over the rounds of the round's
median, "spread" the range of the round medians relative to it.

    python tools/varlen_window_probe.py [--rounds 5] [--reps 10] [--out profiles/varlen_window_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sageattention_amd as sa  # noqa: E402
from sageattention_amd import core  # noqa: E402

HQ, HKV, D = 32, 8, 128
RESIDENT = 512                      # workgroups of a D = 128 kernel the device holds: 256 CUs x 2
WINDOWS = (4096, 1024, 256)
WMAX = 2 ** 30 - 1


def mix():
    g = torch.Generator().manual_seed(12)
    pairs = [(512, n) for n in (2048, 3072, 4096, 5120, 6144, 8192)]
    pairs += [(1, int(n)) for n in torch.randint(1024, 8193, (64,), generator=g)]
    pairs.append((2048, 2048))
    return pairs


def _cdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def tiles_of_item(lq, lk, W, j):
    """(tiles run, head tiles among them) of query block j: sage_attn_kernel's bounds; W = 0: no window."""
    s = lk - lq
    kc0 = 0
    if W > 0:
        a0 = (s - W) + 128 * j + 1
        kc0 = (a0 & ~63) if a0 > 0 else 0
    lk2 = max(lk - kc0, 0)
    kchunk0 = kc0 - s
    n = min(max(_cdiv(128 * j + 128 - kchunk0 + 63, 64), 0), _cdiv(lk2 + 63, 64))
    nh = 0
    if W > 0:
        x = min(128 * j + 127, lq - 1) - kchunk0 + 1 - W
        nh = min((x + 63) >> 6 if x > 0 else 0, n)
    return n, nh


def geometry(pairs, W):
    attended = sum(sum(max(0, min(lk, i + lk - lq + 1) - (max(0, i + lk - lq + 1 - W) if W else 0)) for i in range(lq)) for lq, lk in pairs) * HQ
    items = sum((lq + 127) // 128 for lq, _ in pairs) * HQ
    t = [tiles_of_item(lq, lk, W, j) for lq, lk in pairs for j in range((lq + 127) // 128)]
    return attended, items, sum(x[0] for x in t) * HQ, sum(x[1] for x in t) * HQ


def cu(lens, dev):
    return torch.nn.functional.pad(torch.tensor(lens).cumsum(0), (1, 0)).to(torch.int32).to(dev)


def packed_inputs(pairs, dev, seed):
    g = torch.Generator().manual_seed(seed)
    lq, lk = [p[0] for p in pairs], [p[1] for p in pairs]
    q = torch.randn(sum(lq), HQ, D, generator=g).to(torch.bfloat16).to(dev)
    k, v = (torch.randn(sum(lk), HKV, D, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    return q, k, v, cu(lq, dev), cu(lk, dev), max(lq), max(lk)


def packed_variant(ins, W):
    q, k, v, cq, ck, mq, mk = ins
    kw = dict(window_size=(W - 1, 0)) if W else {}
    call = lambda: sa.sageattn_qk_int8_pv_fp8_varlen(q, k, v, cq, ck, mq, mk, is_causal=True, causal_align="bottom_right", **kw)
    st = core._varlen_prepare(q, k, v, cq, ck, mq, mk, True, None, True, {}, v_fp8=True, bottom_right=True, window=W)
    return call, (lambda: core._varlen_attend_f8(st, True, False))


def dense_inputs(pairs, ins, dev):
    q, k, v = ins[:3]
    B, mq, mk = len(pairs), max(p[0] for p in pairs), max(p[1] for p in pairs)
    qd = torch.zeros(B, HQ, mq, D, dtype=q.dtype, device=dev)
    kd, vd = (torch.zeros(B, HKV, mk, D, dtype=q.dtype, device=dev) for _ in range(2))
    aq = ak = 0
    for b, (lq, lk) in enumerate(pairs):
        qd[b, :, mq - lq:] = q[aq:aq + lq].transpose(0, 1)             # right-aligned: the padded q's last row is the sequence's last row
        kd[b, :, :lk] = k[ak:ak + lk].transpose(0, 1)
        vd[b, :, :lk] = v[ak:ak + lk].transpose(0, 1)
        aq, ak = aq + lq, ak + lk
    lens = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=dev)
    _, _, k8, ks, vimg, vs, _ = core._prepass_kv(qd, kd, vd, "HND", "per_thread", 64, True, False, False, False, kv_lens=lens)
    qs = core._q_start_tensor(None, lens, B, mq, mk, dev)
    return qd, kd, vd, lens, k8, ks, vimg, vs, qs


def dense_variant(dn, W):
    qd, kd, vd, lens, k8, ks, vimg, vs, qs = dn
    call = lambda: sa.sageattn_qk_int8_pv_fp8_cuda(qd, kd, vd, is_causal=True, pv_accum_dtype="fp32+fp32", kv_lens=lens, causal_align="bottom_right",
                                                   window_size=(W - 1, 0))
    sm = core._sm_log2(D ** -0.5)
    return call, (lambda: core._attn_fused_q(qd, k8, vimg, vs, ks, "HND", True, sm, False, kv_lens=lens, q_start=qs, window=W))


def time_interleaved(fns, rounds, reps):
    """us per call: {variant: [median of round 0, round 1, ...]}"""
    per_round = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record(); b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            per_round[n].append(statistics.median(ts))
    return per_round


def summary(per_round):
    out = {}
    for n, xs in per_round.items():
        med = statistics.median(xs)
        out[n] = {"us": round(med, 1), "spread": round((max(xs) - min(xs)) / med, 4), "us_rounds": [round(x, 1) for x in xs]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varlen_window_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "varlen_window_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    pairs = mix()
    ins = packed_inputs(pairs, dev, 13)
    dn = dense_inputs(pairs, ins, dev)
    variants = {"packed": 0, "packed_wmax": WMAX, **{f"packed_w{W}": W for W in WINDOWS}}
    calls, kernels, geo = {}, {}, {}
    for name, W in variants.items():
        calls[name], kernels[name] = packed_variant(ins, W)
        geo[name] = geometry(pairs, W)
    for W in WINDOWS:
        calls[f"dense_w{W}"], kernels[f"dense_w{W}"] = dense_variant(dn, W)
        geo[f"dense_w{W}"] = geo[f"packed_w{W}"]
    # sanity before timing: a window that cuts no row gives the unwindowed bits, and the two routes agree on the windowed rows as closely as
    # their different quantisation groups allow (tools/varlen_br_probe.py: 2^-3 of the largest output)
    assert torch.equal(calls["packed"](), calls["packed_wmax"]()), "W = 2^30 - 1 changed the output"
    worst = {}
    for W in WINDOWS:
        o_p, o_d = calls[f"packed_w{W}"](), calls[f"dense_w{W}"]()
        at, w, top = 0, 0.0, float(o_p.float().abs().max())
        for b, (lq, _) in enumerate(pairs):
            w = max(w, float((o_p[at:at + lq].transpose(0, 1).float() - o_d[b, :, o_d.shape[2] - lq:].float()).abs().max()))
            at += lq
        assert w <= top / 8, f"W = {W}: the packed and the dense call disagree (max|diff| {w}, max|o| {top})"
        worst[W] = w
    r_calls = summary(time_interleaved(calls, a.rounds, a.reps))
    r_kernels = summary(time_interleaved(kernels, a.rounds, a.reps))
    for r in (r_calls, r_kernels):
        for n in list(r):
            attended, items, tiles, head = geo[n]
            r[n]["ps_per_row_key_pair"] = round(r[n]["us"] * 1e6 / attended, 4)
        for n in variants:
            if n != "packed":
                r[n]["over_packed"] = round(r[n]["us"] / r["packed"]["us"], 3)
        for W in WINDOWS:
            r[f"dense_w{W}"]["over_packed_same_window"] = round(r[f"dense_w{W}"]["us"] / r[f"packed_w{W}"]["us"], 3)
    for n in variants:
        attended, items, tiles, head = geo[n]
        r_kernels[n].update(tiles=tiles, head_tiles=head, tiles_per_item=round(tiles / items, 2),
                            us_per_item_resident=round(r_kernels[n]["us"] * RESIDENT / items, 3))
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); GQA 32 / 8, D = 128, bf16, causal "
                   "bottom-right; call = whole entry point, kernel = attention launch alone; spread = range of the round medians / the figure; "
                   "tiles = 64-key tiles from the kernel's loop bounds x Hq; us_per_item_resident = kernel us x 512 resident workgroups / items",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "sequences": pairs,
           "work_items": geo["packed"][1], "attended_row_key_pairs": {n: geo[n][0] for n in variants},
           "max_abs_diff_packed_vs_dense": worst, "call": r_calls, "kernel": r_kernels}
    print(json.dumps({k: res[k] for k in ("work_items", "attended_row_key_pairs", "call", "kernel")}, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
