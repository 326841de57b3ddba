#!/usr/bin/env python3
"""What the packed route's bottom-right causal alignment costs on a serving mix, against what a caller had before it: whole calls and the
attention kernel alone, interleaved.

  packed_br   sageattn_qk_int8_pv_fp8_varlen(..., is_causal=True, causal_align="bottom_right")      (the new route: one packed call)
  dense_br    sageattn_qk_int8_pv_fp8_cuda(q_padded, k_padded, v_padded, is_causal=True, kv_lens=Lk_b, causal_align="bottom_right")
              the same batch padded to [B, H, max Lq, D] / [B, H, max Lk, D], every sequence's rows right-aligned in its padded q so that
              its last row sees its last key -- the dense kv_lens route of DESIGN.md 3.10

Mix (GQA 32 / 8, D = 128, bf16): six chunks of 512 rows against 2048 ... 8192 cached keys, 64 decode rows (Lq = 1) against 1024 ... 8192 keys
(seeded), one full 2048-row prefill.  Next to the times: the (row, key) pairs the mask attends to and ps per pair (DESIGN.md 3.10 has 0.49 for
the dense route at its chunked-prefill shape), the 64-key tiles the kernel's loop bounds give (sum of the work list's weights x Hq), and an
estimate of what a work item costs outside its tiles: (kernel time x resident workgroups - tiles x t_tile) / items, with t_tile taken from one
long packed causal sequence (16384 rows, the same heads) through the same kernels, where the items' fixed part is small against their tiles.

"call" is the whole entry point (plan + pre-pass + attention); "kernel" is the attention launch alone on operands prepared once.  Per round
every variant is warmed, then timed call by call with device events; the figure of a variant is the median over the rounds of the round's
median, "spread" the range of the round medians relative to it.

    python tools/varlen_br_probe.py [--rounds 5] [--reps 10] [--out profiles/varlen_br_probe.json]
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


def mix():
    g = torch.Generator().manual_seed(12)
    pairs = [(512, n) for n in (2048, 3072, 4096, 5120, 6144, 8192)]
    pairs += [(1, int(n)) for n in torch.randint(1024, 8193, (64,), generator=g)]
    pairs.append((2048, 2048))
    return pairs


def weight(lq, lk, j):
    return min(max(-((-(lk - lq + 128 * (j + 1))) // 64), 0), -(-lk // 64))


def geometry(pairs):
    attended = sum(sum(max(0, min(lk, i + lk - lq + 1)) for i in range(lq)) for lq, lk in pairs) * HQ
    items = sum((lq + 127) // 128 for lq, _ in pairs) * HQ
    tiles = sum(weight(lq, lk, j) for lq, lk in pairs for j in range((lq + 127) // 128)) * HQ
    return attended, items, tiles


def cu(lens, dev):
    return torch.nn.functional.pad(torch.tensor(lens).cumsum(0), (1, 0)).to(torch.int32).to(dev)


def packed_variant(pairs, dev, seed, **kw):
    g = torch.Generator().manual_seed(seed)
    lq, lk = [p[0] for p in pairs], [p[1] for p in pairs]
    q = torch.randn(sum(lq), HQ, D, generator=g).to(torch.bfloat16).to(dev)
    k, v = (torch.randn(sum(lk), HKV, D, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    cq, ck = cu(lq, dev), cu(lk, dev)
    call = lambda: sa.sageattn_qk_int8_pv_fp8_varlen(q, k, v, cq, ck, max(lq), max(lk), is_causal=True, **kw)
    st = core._varlen_prepare(q, k, v, cq, ck, max(lq), max(lk), True, None, True, {}, v_fp8=True,
                              bottom_right=kw.get("causal_align") == "bottom_right")
    kernel = lambda: core._varlen_attend_f8(st, True, False)
    return call, kernel, (q, k, v)


def dense_variant(pairs, packed_qkv, dev):
    q, k, v = packed_qkv
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
    call = lambda: sa.sageattn_qk_int8_pv_fp8_cuda(qd, kd, vd, is_causal=True, pv_accum_dtype="fp32+fp32", kv_lens=lens, causal_align="bottom_right")
    _, _, k8, ks, vimg, vs, _ = core._prepass_kv(qd, kd, vd, "HND", "per_thread", 64, True, False, False, False, kv_lens=lens)
    qs = core._q_start_tensor(None, lens, B, mq, mk, dev)
    sm = core._sm_log2(D ** -0.5)
    kernel = lambda: core._attn_fused_q(qd, k8, vimg, vs, ks, "HND", True, sm, False, kv_lens=lens, q_start=qs)
    return call, kernel


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varlen_br_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "varlen_br_probe.py measures on the GPU"
    dev = torch.device("cuda:0")
    pairs = mix()
    attended, items, tiles = geometry(pairs)
    p_call, p_kernel, qkv = packed_variant(pairs, dev, 13, causal_align="bottom_right")
    d_call, d_kernel = dense_variant(pairs, qkv, dev)
    long_pairs = [(16384, 16384)]
    _, l_kernel, _ = packed_variant(long_pairs, dev, 14, causal_align="bottom_right")
    _, l_items, l_tiles = geometry(long_pairs)
    # the two routes compute the same rows with different quantisation groups (per-block against per-thread Q and K scales, V scales per sequence
    # against per padded sample): close, not equal.  A row that sees one key returns that V row, rounded to e4m3 under either scale -- two
    # roundings of 2^-4 relative each -- so the sanity bar is 2^-3 of the largest output
    o_p, o_d = p_call(), d_call()
    at, worst = 0, 0.0
    top = float(o_p.float().abs().max())
    for b, (lq, _) in enumerate(pairs):
        worst = max(worst, float((o_p[at:at + lq].transpose(0, 1).float() - o_d[b, :, o_d.shape[2] - lq:].float()).abs().max()))
        at += lq
    assert worst <= top / 8, f"the packed and the dense call disagree (max|diff| {worst}, max|o| {top})"
    calls = summary(time_interleaved({"packed_br": p_call, "dense_br": d_call}, a.rounds, a.reps))
    kernels = summary(time_interleaved({"packed_br": p_kernel, "dense_br": d_kernel, "packed_long_causal": l_kernel}, a.rounds, a.reps))
    t_tile = kernels["packed_long_causal"]["us"] * RESIDENT / l_tiles
    for r in (calls, kernels):
        for n in ("packed_br", "dense_br"):
            r[n]["ps_per_row_key_pair"] = round(r[n]["us"] * 1e6 / attended, 4)
        r["dense_over_packed"] = round(r["dense_br"]["us"] / r["packed_br"]["us"], 3)
    res = {"what": "us per call, median over interleaved rounds of the round's median (device events); GQA 32 / 8, D = 128, bf16, causal "
                   "bottom-right; call = whole entry point, kernel = attention launch alone; spread = range of the round medians / the figure",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "sequences": pairs,
           "attended_row_key_pairs": attended, "work_items": items, "tiles_from_loop_bounds": tiles, "max_abs_diff_packed_vs_dense": worst,
           "call": calls, "kernel": kernels,
           "per_item": {"us_per_tile_long_sequence": round(t_tile, 4), "long_sequence_items": l_items, "long_sequence_tiles": l_tiles,
                        "tiles_per_item": round(tiles / items, 2), "us_of_tiles_at_that_rate": round(tiles * t_tile / RESIDENT, 1),
                        "us_per_item_outside_its_tiles": round((kernels["packed_br"]["us"] * RESIDENT - tiles * t_tile) / items, 3)}}
    print(json.dumps({k: res[k] for k in ("attended_row_key_pairs", "work_items", "tiles_from_loop_bounds", "call", "kernel", "per_item")}, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
