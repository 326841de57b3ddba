"""CPU: the order in which the KV caches' three C entries check their arguments (``sage_kvcache_append``, ``sage_kvpaged_append``,
``sage_kvpaged_attn``).  A call that breaks two rules reports the rule the entry checks first; the entries share their checks' code but not
their order (the contiguous append tests ``head_dim`` and ``T`` before ``B`` / ``Hkv``, the paged one the page geometry and ``B`` / ``Hkv``
first, and the table's alignment after the 16-byte alignment), so each entry's order is written out here, one violation per check."""
import itertools

import pytest

import util  # noqa: F401  (sys.path)
import test_kv_cache_host as contiguous
import test_paged_kv_host as paged
from sageattention_amd import _cabi, _cabi_kvcache, _cabi_kvpaged


# per entry: (one violating keyword set, a substring of its message), in the order the entry checks; `p` is an aligned address
def _kvcache_append_order(p):
    return [(dict(k_int8=None), b"null cache pointer"),
            (dict(k_new=None), b"null k_new / v_new"),
            (dict(head_dim=96), b"head_dim must be 64 or 128"),
            (dict(T=0), b"T must be at least 1"),
            (dict(capacity=100), b"capacity must be a positive multiple of 64"),
            (dict(B=0), b"B and Hkv"),
            (dict(dtype=2), b"bad dtype"),
            (dict(v_image=p + 2), b"16-byte aligned"),
            (dict(k_sl=68), b"multiples of 8 elements")]


def _kvpaged_append_order(p):
    return [(dict(k_int8=None), b"null cache pointer"),
            (dict(k_new=None), b"null k_new / v_new"),
            (dict(block_table=None), b"null block_table"),
            (dict(page_size=96), b"page_size must be 64 * 2^k"),
            (dict(num_pages=0), b"num_pages must be at least 1"),
            (dict(max_pages_per_seq=0), b"max_pages_per_seq must be at least 1"),
            (dict(B=0), b"B and Hkv"),
            (dict(head_dim=96), b"head_dim must be 64 or 128"),
            (dict(T=0), b"T must be at least 1"),
            (dict(dtype=2), b"bad dtype"),
            (dict(v_image=p + 2), b"16-byte aligned"),
            (dict(block_table=p + 2), b"block_table must be 4-byte aligned"),
            (dict(k_sl=68), b"multiples of 8 elements")]


def _kvpaged_attn_order(p):
    return [(dict(q=None), b"null tensor pointer"),
            (dict(kv_lens=None), b"null kv_lens"),
            (dict(block_table=None), b"null block_table"),
            (dict(page_size=96), b"page_size must be 64 * 2^k"),
            (dict(num_pages=0), b"num_pages must be at least 1"),
            (dict(max_pages_per_seq=0), b"max_pages_per_seq must be at least 1"),
            (dict(B=0), b"B and Hkv"),
            (dict(block_table=p + 2), b"block_table must be 4-byte aligned"),
            (dict(attr=_cabi.launch_attr(folded_scores=True)), b"SAGE_ATTR_FP8_FOLDED_SCORES is not supported on a paged cache"),
            (dict(D=96), b"head_dim must be 64 or 128"),
            (dict(Lq=0), b"empty problem"),
            (dict(Hq=3, Hkv=2), b"divisible"),
            (dict(q_dtype=2), b"bad q_dtype"),
            (dict(out_dtype=-1), b"bad out_dtype"),
            (dict(o=p + 2), b"16-byte aligned"),
            (dict(q_sl=68), b"q strides"),
            (dict(k_sl=72), b"k strides"),
            (dict(o_sh=4), b"output strides")]


ENTRIES = {"sage_kvcache_append": (_cabi_kvcache, contiguous._append, _kvcache_append_order),
           "sage_kvpaged_append": (_cabi_kvpaged, paged._append, _kvpaged_append_order),
           "sage_kvpaged_attn": (_cabi_kvpaged, paged._attn, _kvpaged_attn_order)}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_two_violations_report_the_earlier_check(entry):
    binding, call, order = ENTRIES[entry]
    lib = binding.load()
    buf, p = paged._aligned_buffer()
    checks = order(p)
    for kw, match in checks:                                         # each violation alone gives its own message
        rc, msg = call(lib, p, **kw)
        assert rc == -1 and match in msg, (entry, kw, rc, msg)
    covered = set()
    for (i, (kw_i, match_i)), (j, (kw_j, _)) in itertools.combinations(enumerate(checks), 2):
        if set(kw_i) & set(kw_j):                                    # two values for one argument do not fit into one call
            continue
        rc, msg = call(lib, p, **kw_i, **kw_j)
        assert rc == -1 and match_i in msg, (entry, kw_i, kw_j, rc, msg)
        covered.add((i, j))
    # the cap on what may be skipped: every adjacent pair of checks is on distinct arguments, so every step of the order is pinned
    assert all((i, i + 1) in covered for i in range(len(checks) - 1)), (entry, sorted(covered))
    del buf
