"""Where the pages of the 4 GiB+ pool test lie, and the program it runs -- TEST INFRASTRUCTURE ONLY, pure Python.

tests/test_gpu_kv_large_pool.py builds a ``PagedQuantizedKVCache`` whose ``k_int8`` and ``v_image`` are 4.5 GiB each, so that a page, a K scale
slot or a V-image tile can lie at a byte offset of 2^31 or 2^32 and more from its tensor's base, and runs a serving program on it and on a
64-page TWIN with the same logical table.  This module decides, without a GPU, which pages the sequences own -- on both sides of the signed
and the unsigned 32-bit boundary, at the bottom and at the very top of the pool -- and checks nothing itself: tests/test_kv_large_pool_host.py
asserts the placement, the GPU file imports it.

With ``P = Hkv * page_size * D`` bytes per page of ``k_int8`` (and of ``v_image``): ``N31 = 2^31 / P`` is the first page at a signed-negative
32-bit byte offset, ``N32 = 2^32 / P`` the first whose offset does not fit 32 bits, ``num_pages = N32 + N32 / 8``.  An address product that
lost its 64-bit cast would reach, for a page ``g >= N32``, the ALIAS page ``g - N32``; no alias is ever assigned, so such a store lands in
poison and such a load reads poison.
"""
import collections

POISON = 0x5A
NSLOTS = 8                                  # four prompts (slots 0 .. 3) and four fork children (4 .. 7)
TWIN_PAGES = 64

Geometry = collections.namedtuple("Geometry", "name D Hkv page_size cap contexts P N31 N32 num_pages")


def geometry(name):
    D, Hkv, page_size, cap, contexts = {"a": (128, 8, 256, 4096, (3000, 1061, 256, 0)), "b": (64, 2, 64, 1536, (1061, 257, 64, 0))}[name]
    P = Hkv * page_size * D
    assert 2 ** 31 % P == 0
    N32 = 2 ** 32 // P
    return Geometry(name, D, Hkv, page_size, cap, contexts, P, 2 ** 31 // P, N32, N32 + N32 // 8)


# the program: every mutating call, in order.  Counts are per slot.
SINGLE_ROWS = 3                             # slot 2 holds exactly one page: the first of three one-row appends opens its second, a high page
VARLEN_COUNTS = (5, 0, 3, 70, 0, 0, 0, 0)
FORKS = ((2, 4), (2, 5), (1, 6), (0, 7))    # (parent, child)
FORK_PREFIX = {7: 700}                      # child 7 takes a prefix: rounded down to 640 keys
CHILD_COUNTS = (2, 0, 1, 0, 251, 3, 5, 70)  # the last dense append: parents and children go their own ways; child 4 crosses into further pages


def regions(g):
    return dict(low=(2, 3, 5, 6), signed=(g.N31 - 1, g.N31, g.N31 + 1), unsigned=(g.N32 - 1, g.N32, g.N32 + 1, g.N32 + 7), top=(g.num_pages - 1,))


def _prefix_len(L, prefix):
    if prefix is None:
        return L
    p = max(0, min(prefix, L))
    return p & ~63 if p < L else p


def lens_after(g):
    """The lengths after each mutating call: [(name, lens)]."""
    lens = list(g.contexts) + [0] * (NSLOTS - 4)
    out = [("prompts", tuple(lens))]
    for i in range(SINGLE_ROWS):
        lens[2] += 1
        out.append((f"single row {i}", tuple(lens)))
    lens = [n + c for n, c in zip(lens, VARLEN_COUNTS)]
    out.append(("append_varlen", tuple(lens)))
    for s, d in FORKS:
        lens[d] = _prefix_len(lens[s], FORK_PREFIX.get(d))
    out.append(("fork", tuple(lens)))
    lens = [n + c for n, c in zip(lens, CHILD_COUNTS)]
    out.append(("children", tuple(lens)))
    assert max(lens) <= g.cap
    return out


def placement(g):
    """(table, fork_pages): ``table[b]`` the page ids of slot b's entries as the caller writes them BEFORE the program (None: an entry no tile
    needs, which takes junk), ``fork_pages[child]`` the page a fork gives the child as its first own.  Prompts take their pages round-robin from
    an order that walks the regions out of order; the children's further pages come from the same order."""
    ps, max_pages = g.page_size, g.cap // g.page_size
    steps = dict(lens_after(g))
    before_fork, final = steps["append_varlen"], steps["children"]
    need = [-(-n // ps) for n in final]
    listed = [g.N32, 3, g.N31, g.N32 - 1, 2, g.N31 - 1]
    fill = [x for i in range(40) for x in (g.N32 + 8 + i, 100 + 3 * i, g.N31 + 2 + i, g.num_pages - 2 - i)]
    order = iter(listed + fill)
    table = [[None] * max_pages for _ in range(NSLOTS)]
    # slot 2's second page -- opened by a single-row append -- lies just past 2^32 bytes; slot 1's open page is a low one
    table[2][1] = g.N32 + 7
    table[1][need[1] - 1] = 5
    for e in range(max_pages):
        for b in range(4):
            if e < need[b] and table[b][e] is None:
                table[b][e] = next(order)
    # the forks: parent's open page high -> one child low, one at the top of the pool; parent low -> child high; a prefix -> just past 2^31
    fork_pages = {4: 6, 5: g.num_pages - 1, 6: g.N32 + 1, 7: g.N31 + 1}
    first_own = {}
    for s, d in FORKS:
        P = _prefix_len(before_fork[s], FORK_PREFIX.get(d))
        first_own[d] = P // ps                              # the entry the fork writes; the entries in front are the parent's
        for e in range(first_own[d] + 1, need[d]):
            table[d][e] = next(order)
    return table, fork_pages, first_own


def assigned_pages(g):
    table, fork_pages, _ = placement(g)
    return sorted({p for row in table for p in row if p is not None} | set(fork_pages.values()))


def aliases(g):
    """{alias page: the assigned page it stands for} of every assigned page at 2^32 bytes or beyond."""
    return {p - g.N32: p for p in assigned_pages(g) if p >= g.N32}


def twin_id(g):
    """big page id -> twin page id: injective into [0, TWIN_PAGES), neither ascending nor the identity on the low pages."""
    pages = assigned_pages(g)
    assert len(pages) <= TWIN_PAGES
    return {p: (29 * i + 11) % TWIN_PAGES for i, p in enumerate(pages)}


def junk(num_pages, i):
    return (-1, num_pages)[i % 2]


def tables(g):
    """(big table, twin table) as lists ``[NSLOTS][max_pages]`` in front of the program: the same logical table; entries no tile needs hold -1
    and ``num_pages`` in turn (the twin's: its own ``num_pages``).  The entry a fork writes is junk until it does."""
    table, _, _ = placement(g)
    tid = twin_id(g)
    big, twin, j = [], [], 0
    for row in table:
        rb, rt = [], []
        for p in row:
            if p is None:
                rb.append(junk(g.num_pages, j))
                rt.append(junk(TWIN_PAGES, j))
                j += 1
            else:
                rb.append(p)
                rt.append(tid[p])
        big.append(rb)
        twin.append(rt)
    return big, twin


# ---- the contiguous cache: B 72 slabs of 64 MiB of k_int8 each (Hkv 8, D 128, capacity 65536), 4.5 GiB per tensor
CONTIGUOUS = dict(B=72, Hkv=8, D=128, cap=65536, twin_cap=1536,
                  lens={2: 300, 31: 257, 32: 64, 63: 449, 64: 320, 65: 1, 71: 513})      # slot -> keys; every other slot stays empty


def contiguous_aliases():
    c = CONTIGUOUS
    slab = c["Hkv"] * c["cap"] * c["D"]
    n32 = 2 ** 32 // slab
    return {b - n32: b for b in c["lens"] if b >= n32}
