"""CPU: the kv_lens family's keywords (``num_splits``, ``pack_gqa``, ``kv_lens``, ``window_size``, ``q_start`` / ``causal_align``) are resolved
once, for ``sageattn_qk_int8_pv_fp8_cuda`` and ``sageattn_kvcache`` alike -- which keyword's error a call that breaks two rules gets, that the
two entry points word it the same, that a window alone takes both to the same point, and that the resolved record of a call with one keyword
differs from the plain call's in that keyword's fields only (what lets one route body serve every combination)."""
import pytest
import torch

import util  # noqa: F401  (sys.path)
from sageattention_amd import core as sc
from sageattention_amd.kv_cache import QuantizedKVCache, sageattn_kvcache
from test_kv_split_host import _cpu_qkv

ORDER = ["num_splits", "pack_gqa", "kv_lens", "window_size", "q_start", "split_kv_exact"]
BOTH_OFFSETS = dict(q_start=0, causal_align="bottom_right")

# (shape deviations from _cpu_qkv's defaults, keywords, the keyword whose error the call gets, a piece of that error)
PRECEDENCE = {
    "num_splits>pack_gqa": (dict(Lq=129), dict(num_splits=2, pack_gqa=True), "num_splits", "num_splits needs qo_len <= 128"),
    "num_splits>kv_lens": (dict(Lq=129), dict(num_splits=2, kv_lens=torch.zeros(3, dtype=torch.int32)), "num_splits", "num_splits needs qo_len <= 128"),
    "pack_gqa>kv_lens": (dict(Hq=2, Hkv=2), dict(pack_gqa=True, kv_lens=torch.zeros(2)), "pack_gqa", "no GQA group to pack"),
    "kv_lens>window_size": (dict(), dict(kv_lens=torch.zeros(3, dtype=torch.int32), window_size=(5, 7), is_causal=True), "kv_lens", r"kv_lens must have shape \[B\]"),
    "window_size>q_start": (dict(), dict(window_size=(5, 7), is_causal=True, **BOTH_OFFSETS), "window_size", "right must be 0 or -1"),
    # a well-formed window breaks no rule of its own; it turns the call causal in front of the offsets' check, which therefore refuses the
    # pair of offsets and not a non-causal call
    "window_size,q_start": (dict(), dict(window_size=(5, 0), **BOTH_OFFSETS), "q_start", "pass either q_start or causal_align='bottom_right'"),
    "q_start>split_kv_exact": (dict(), dict(is_causal=True, q_start=torch.zeros(3, dtype=torch.int32), split_kv_exact=True, pv_accum_dtype="fp32"),
                               "q_start", r"q_start must have shape \[B\]"),
}
SHARED = [n for n, (_, kw, _, _) in PRECEDENCE.items() if "kv_lens" not in kw and "split_kv_exact" not in kw]


def _cache():
    c = QuantizedKVCache.allocate(2, 2, 100, 64, torch.float16, "cpu")
    return c.seed(torch.zeros(2, 2, 64, dtype=torch.float16), torch.ones(2, 2, 64))


def _error(fn, *args, **kw) -> str:
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    return str(e.value)


@pytest.mark.parametrize("case", list(PRECEDENCE))
def test_a_call_that_breaks_two_rules_gets_the_earlier_keywords_error(case):
    shape, kw, first, piece = PRECEDENCE[case]
    q, k, v = _cpu_qkv(**shape)
    with pytest.raises(ValueError, match=piece) as e:
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, **kw)
    msg = str(e.value)
    assert first in msg and not any(later in msg for later in ORDER[ORDER.index(first) + 1:]), msg


def test_the_cases_are_in_the_family_order():
    assert [PRECEDENCE[c][2] for c in PRECEDENCE] == ["num_splits", "num_splits", "pack_gqa", "kv_lens", "window_size", "q_start", "q_start"]
    assert SHARED == ["num_splits>pack_gqa", "window_size>q_start", "window_size,q_start"]


@pytest.mark.parametrize("case", SHARED)
def test_the_cache_raises_the_entry_points_error(case):
    shape, kw, _, _ = PRECEDENCE[case]
    q, k, v = _cpu_qkv(**shape)
    assert _error(sageattn_kvcache, q, _cache(), **kw) == _error(sc.sageattn_qk_int8_pv_fp8_cuda, q, k, v, **kw)


def test_a_window_alone_takes_both_entry_points_past_the_keywords():
    """``window_size=(5, 0)`` on a non-causal call without offsets: the window makes the call causal and the offsets 0, so neither entry point
    refuses it ("needs is_causal=True" is what the offsets' check says of a non-causal call) and both go on to their first device step -- the
    entry point's input check, the cache's device selection -- which is where a CPU tensor ends."""
    q, k, v = _cpu_qkv()
    with pytest.raises(AssertionError, match="cuda"):
        sc.sageattn_qk_int8_pv_fp8_cuda(q, k, v, window_size=(5, 0))
    with pytest.raises(Exception) as e:
        sageattn_kvcache(q, _cache(), window_size=(5, 0))
    assert "is_causal" not in str(e.value) and "window_size" not in str(e.value) and "cuda" in str(e.value).lower()
    with pytest.raises(Exception) as plain:                    # the call without the keyword ends at the same step
        sageattn_kvcache(q, _cache())
    assert type(e.value) is type(plain.value) and str(e.value) == str(plain.value)


def test_one_keyword_moves_its_own_fields_only():
    """The record of a call with ``pack_gqa``, ``num_splits`` or an offset alone is the plain call's but for that keyword's fields: the one route
    body needs no case of its own for any of them."""
    q, k, _ = _cpu_qkv()

    def record(is_causal=False, kv_lens=None, q_start=None, causal_align="top_left", window_size=None, pack_gqa=None, num_splits=None):
        return sc._kv_family_args(q, k, "HND", is_causal, kv_lens, q_start, causal_align, window_size, pack_gqa, num_splits,
                                  "per_thread", "fp32+fp16", False, {})

    plain = record()
    assert plain == (False, 0, 0, False, 0, False, False, None)
    assert plain._fields == ("is_causal", "window", "shift", "gqa_pack", "splits", "with_lens", "with_start", "q_start")
    assert record(pack_gqa=True) == plain._replace(gqa_pack=True)
    assert record(num_splits=2) == plain._replace(splits=2)
    assert record(is_causal=True, q_start=0) == plain._replace(is_causal=True, with_start=True, q_start=0)
    assert record(window_size=(5, 0)) == plain._replace(is_causal=True, window=6, with_start=True, q_start=0)
    assert record(window_size=(5, 7)) == plain._replace(is_causal=True, window=13, shift=7, with_start=True, q_start=0)
    with pytest.raises(AttributeError):
        plain.splits = 2
