"""CPU: the placement and alias arithmetic of the 4 GiB+ pool test (tests/kv_large_pool_plan.py, run by tests/test_gpu_kv_large_pool.py)."""
import pytest

import kv_large_pool_plan as plan


@pytest.mark.parametrize("name", ["a", "b"])
def test_the_geometry_is_what_the_test_says(name):
    g = plan.geometry(name)
    assert g.P == g.Hkv * g.page_size * g.D and g.N31 * g.P == 2 ** 31 and g.N32 * g.P == 2 ** 32
    assert g.num_pages * g.P == 4 * 2 ** 30 + 2 ** 29                    # 4.5 GiB of k_int8, and as much of v_image
    assert (g.P, g.num_pages) == {"a": (256 * 1024, 18432), "b": (8 * 1024, 589824)}[name]
    assert g.num_pages - 1 < 2 ** 31 and g.cap % g.page_size == 0


@pytest.mark.parametrize("name", ["a", "b"])
def test_the_sequences_own_pages_in_every_region_and_no_alias(name):
    g = plan.geometry(name)
    table, fork_pages, first_own = plan.placement(g)
    assigned = plan.assigned_pages(g)
    flat = [p for row in table for p in row if p is not None] + list(fork_pages.values())
    assert len(flat) == len(set(flat)) == len(assigned), "a page is handed out twice"
    assert all(0 <= p < g.num_pages for p in assigned)
    for region, pages in plan.regions(g).items():
        assert set(pages) <= set(assigned), (region, sorted(set(pages) - set(assigned)))
    # every alias -- the page 4 GiB below an assigned page -- is unassigned; that is why pages 0, 1 and 7 stay free
    al = plan.aliases(g)
    assert {0, 1, 7, g.N32 // 8 - 1} <= set(al) and len(al) >= 8
    assert not set(al) & set(assigned), sorted(set(al) & set(assigned))
    # every prompt slot owns pages below 2^31 bytes, between 2^31 and 2^32, and at or beyond 2^32, or (the short ones) on one side each
    side = lambda p: 0 if p < g.N31 else 1 if p < g.N32 else 2
    assert {side(p) for p in table[0] if p is not None} == {0, 1, 2}
    assert {side(p) for b in (1, 2, 3) for p in table[b] if p is not None} == {0, 1, 2}
    # interleaved and not ascending
    own0, own1 = [p for p in table[0] if p is not None], [p for p in table[1] if p is not None]
    assert own0 != sorted(own0) and min(own1) < max(own0) and min(own0) < max(own1)
    # the forks: parent's open page high -> children low and at the top; parent low -> child high; the prefix child just past 2^31
    before = dict(plan.lens_after(g))["append_varlen"]
    open_page = lambda b: table[b][(before[b] - 1) // g.page_size]
    assert before[2] % g.page_size and open_page(2) == g.N32 + 7 and fork_pages[4] == 6 and fork_pages[5] == g.num_pages - 1
    assert before[1] % g.page_size and open_page(1) == 5 and fork_pages[6] == g.N32 + 1
    assert fork_pages[7] == g.N31 + 1 and first_own[7] == 640 // g.page_size


@pytest.mark.parametrize("name", ["a", "b"])
def test_every_page_a_sequence_needs_exists_and_the_twin_has_the_same_logical_table(name):
    g = plan.geometry(name)
    table, fork_pages, first_own = plan.placement(g)
    big, twin = plan.tables(g)
    tid = plan.twin_id(g)
    assert len(set(tid.values())) == len(tid) and all(0 <= t < plan.TWIN_PAGES for t in tid.values())
    assert any(tid[p] != i for i, p in enumerate(sorted(tid)))
    # the walk of the program: whenever a slot's length grows, the entries of its tiles are pages (written in front, by a fork, or inherited)
    have = [list(r) for r in table]
    steps = plan.lens_after(g)
    for (what, lens), (_, prev) in zip(steps, [("", (0,) * plan.NSLOTS)] + steps[:-1]):
        if what == "fork":
            for s, d in plan.FORKS:
                have[d][:first_own[d]] = have[s][:first_own[d]]
                have[d][first_own[d]] = fork_pages[d]
            assert lens[7] == 640 and lens[4] == lens[5] == prev[2] and lens[6] == prev[1]
        for b, n in enumerate(lens):
            for e in range(-(-n // g.page_size)):
                assert have[b][e] is not None, (what, b, e)
    # the single rows open slot 2's second page; child 4 crosses from its copy of the open page into a page of its own
    assert steps[0][1][2] == g.page_size and steps[-1][1][4] > 2 * g.page_size
    # big and twin: the same logical table, junk where no tile needs an entry
    for b in range(plan.NSLOTS):
        for e, p in enumerate(table[b]):
            if p is None:
                assert big[b][e] in (-1, g.num_pages) and twin[b][e] in (-1, plan.TWIN_PAGES)
            else:
                assert big[b][e] == p and twin[b][e] == tid[p]


def test_the_contiguous_slots_and_their_aliases():
    c = plan.CONTIGUOUS
    slab = c["Hkv"] * c["cap"] * c["D"]
    assert slab == 64 * 2 ** 20 and c["B"] * slab == 4 * 2 ** 30 + 2 ** 29
    assert sorted(c["lens"]) == [2, 31, 32, 63, 64, 65, 71] and max(c["lens"].values()) <= c["twin_cap"]
    assert plan.contiguous_aliases() == {0: 64, 1: 65, 7: 71} and not set(plan.contiguous_aliases()) & set(c["lens"])
    assert 31 * slab < 2 ** 31 <= 32 * slab and 63 * slab < 2 ** 32 <= 64 * slab
