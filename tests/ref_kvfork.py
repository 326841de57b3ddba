"""What ``sage_kvfork`` (include/sage_kvfork_gfx950.h) leaves behind, restated in numpy -- the C clamps included.  tests/test_kvfork_host.py
asserts it against cases written out by hand; the GPU tests (tests/test_gpu_kv_fork.py) take their expectations from it.

A cache's state is a dict of numpy arrays, any dtype of the right item size (a test passes integer views, so NaN poison keeps its bits):
  k_int8 [num_pages, H, ps, D]   k_scale [num_pages, H, ps / 64 * 4]   v_image [num_pages, H, ps / 64, D, 64]
  v_scale, v_amax [B, H, D]   k_mean [B, H, D] or None   k_tail, v_tail [B, H, 64, D]   lens int32 [B]   block_table int32 [B, max_pages]
"""
import numpy as np

KEYS = ("k_int8", "k_scale", "v_image", "v_scale", "v_amax", "k_mean", "k_tail", "v_tail", "lens", "block_table")


def prefix_len(L, prefix):
    """P of one fork: ``L`` the parent's clamped length, ``prefix`` None or prefix_lens[i]."""
    if prefix is None:
        return L
    P = min(max(int(prefix), 0), L)
    return P & ~63 if P < L else P


def fork_state(state, page_size, src_slots, dst_slots, new_pages, prefix_lens=None):
    """A copy of ``state`` after ``fork(src_slots, dst_slots, new_pages, prefix_lens)``: the forks one after the other (a call that keeps the
    contract -- destinations distinct and disjoint from the sources, new pages distinct and not live -- gives the same in any order)."""
    out = {k: (None if state[k] is None else np.array(state[k], copy=True)) for k in KEYS}
    num_pages, B, max_pages = out["k_int8"].shape[0], out["lens"].shape[0], out["block_table"].shape[1]
    shift = (page_size // 64).bit_length() - 1
    assert page_size == 64 << shift and out["k_int8"].shape[2] == page_size
    cap = max_pages * page_size
    n = len(src_slots)
    assert len(dst_slots) == n and len(new_pages) == n and (prefix_lens is None or len(prefix_lens) == n)
    for i in range(n):
        s, d, pg = int(src_slots[i]), int(dst_slots[i]), int(new_pages[i])
        if not 0 <= s < B or not 0 <= d < B or s == d:
            continue
        L = min(max(int(out["lens"][s]), 0), cap)
        P = prefix_len(L, None if prefix_lens is None else prefix_lens[i])
        np_, r = P >> (6 + shift), P & (page_size - 1)
        table = out["block_table"]
        sp = int(table[s, np_]) if np_ < max_pages else None          # (read before the row of d is written: s != d)
        table[d, :np_] = table[s, :np_]
        if np_ < max_pages:
            table[d, np_] = pg
        if r > 0 and 0 <= sp < num_pages and 0 <= pg < num_pages:
            t = (r + 63) // 64
            out["k_int8"][pg, :, :64 * t] = out["k_int8"][sp, :, :64 * t]
            out["k_scale"][pg, :, :4 * t] = out["k_scale"][sp, :, :4 * t]
            out["v_image"][pg, :, :t] = out["v_image"][sp, :, :t]
        for k in ("v_scale", "v_amax", "k_mean"):
            if out[k] is not None:
                out[k][d] = out[k][s]
        out["k_tail"][d, :, :P % 64] = out["k_tail"][s, :, :P % 64]
        out["v_tail"][d, :, :P % 64] = out["v_tail"][s, :, :P % 64]
        out["lens"][d] = P
    return out
