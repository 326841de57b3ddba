"""CPU self-tests of tests/fence.py.  A checker that cannot fail is worth nothing: the negative controls here change a guard byte through the
arena tensor itself (ordinary indexing of owned memory) and require ``check()`` to fail with the right site, side and offsets.  The fence is
given a device predicate that lets CPU tensors be fenced for the purpose."""
import re

import pytest
import torch

import fence
from fence import FILLS, GUARD, Fence, FenceViolation

ANY = lambda dev: True


def _rec(f, t):
    p = t.untyped_storage().data_ptr()
    return next(r for r in f.arenas if r.arena.untyped_storage().data_ptr() == p)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.int8, torch.int32, torch.uint8])
def test_layout_alignment_shape_and_fill(fill, dtype):
    with Fence(fill, device_ok=ANY) as f:
        t = torch.empty((3, 5, 7), dtype=dtype, device="cpu")
        z = torch.zeros(11, 2, dtype=dtype)                        # (sizes as varargs, the default device)
        assert t.shape == (3, 5, 7) and t.dtype == dtype and t.is_contiguous() and t.data_ptr() % fence.ALIGN == 0
        assert z.shape == (11, 2) and z.dtype == dtype and z.is_contiguous() and z.data_ptr() % fence.ALIGN == 0
        assert f.owns(t) and f.owns(z) and not f.owns(torch.ones(3))
        assert bool((t.view(torch.uint8) == fill).all()), "the body of an empty holds the fill"
        assert bool((z.view(torch.uint8) == 0).all()), "the body of a zeros stays zero"
        for x in (t, z):
            r = _rec(f, x)
            assert r.nbytes == x.numel() * x.element_size() and r.shape == tuple(x.shape) and r.dtype == dtype
            assert r.arena.data_ptr() + r.lo == x.data_ptr() and r.lo >= GUARD
            (_, lo), (_, hi) = r.guards()
            assert lo.numel() == hi.numel() == GUARD == 64 * 1024
            assert lo.data_ptr() + GUARD == x.data_ptr() and hi.data_ptr() == x.data_ptr() + r.nbytes
            assert bool((lo == fill).all()) and bool((hi == fill).all())
        f.check()
        t.fill_(1)
        z.fill_(1)                                                  # writing every owned element is no violation
        f.check()


def test_the_poison_reads_as_nan_or_minus_one():
    with Fence(0xFF, device_ok=ANY):
        for dt in (torch.float16, torch.bfloat16, torch.float32):
            assert bool(torch.empty(9, dtype=dt).isnan().all())
        assert bool(torch.empty(9, dtype=torch.uint8).view(torch.float8_e4m3fn).float().isnan().all())
        assert bool((torch.empty(9, dtype=torch.int8) == -1).all()) and bool((torch.empty(9, dtype=torch.int32) == -1).all())
    with Fence(0x5A, device_ok=ANY):
        for dt in (torch.float16, torch.bfloat16, torch.float32):
            assert bool(torch.isfinite(torch.empty(9, dtype=dt)).all())


def test_what_passes_through_untouched():
    with Fence(0xFF) as f:                                          # the default predicate: CUDA only
        a = torch.empty(4, 4)
        b = torch.zeros((2, 3), dtype=torch.int32, device="cpu")
        c = torch.empty_like(a)
        assert not f.arenas and b.sum() == 0 and c.shape == a.shape
    with Fence(0xFF, device_ok=ANY) as f:
        assert torch.empty((0,), dtype=torch.float32).numel() == 0 and torch.empty([0]).numel() == 0 and torch.zeros(3, 0).shape == (3, 0)
        out = torch.ones(5)
        torch.zeros(5, out=out)
        assert not f.arenas and out.sum() == 0
        assert torch.empty(3, device="meta").device.type == "meta" and not f.arenas


def test_empty_like_keeps_shape_dtype_and_dense_strides():
    with Fence(0x5A, device_ok=ANY) as f:
        src = torch.arange(2 * 3 * 4 * 8, dtype=torch.float32).view(2, 3, 4, 8)
        a = torch.empty_like(src)
        b = torch.empty_like(src.transpose(1, 2))                   # dense, not contiguous: strides are kept (preserve_format)
        c = torch.empty_like(src[:, :, :2])                         # not dense: contiguous
        d = torch.empty_like(src, dtype=torch.int8)
        assert a.shape == src.shape and a.stride() == src.stride() and f.owns(a)
        assert b.shape == (2, 4, 3, 8) and b.stride() == src.transpose(1, 2).stride() and f.owns(b)
        assert c.shape == (2, 3, 2, 8) and c.is_contiguous() and f.owns(c)
        assert d.dtype == torch.int8 and d.shape == src.shape and f.owns(d)
        assert bool((a.view(torch.uint8) == 0x5A).all())
        f.check()


def test_sites_name_the_package_frame_or_the_caller():
    from sageattention_amd import kernel_api
    with Fence(0xFF, device_ok=ANY) as f:
        kernel_api._no_lse(None)                                    # zero-sized: passes through
        assert f.package_sites() == []
        t = torch.empty(8)
        assert _rec(f, t).site.startswith("test_fence_host.py:") and not _rec(f, t).in_pkg
        from sageattention_amd import ops
        q = torch.zeros(1, 2, 3, 8)
        lse = ops._lse_alloc(q, 1, 1)                               # an allocation made from inside sageattention_amd
        assert lse.shape == (1, 2, 3) and f.owns(lse)
        assert len(f.package_sites()) == 1 and re.fullmatch(r"sageattention_amd/ops\.py:\d+", f.package_sites()[0])
        f.check()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("side,where,want_first,want_last", [
    ("above", [0], "+0", "+0"),                                     # the first byte behind the buffer: a store one element too far
    ("above", [5, GUARD - 1], "+5", f"+{GUARD - 1}"),
    ("below", [-1], "-1", "-1"),                                    # the byte in front of the buffer
    ("below", [-GUARD, -16], f"-{GUARD}", "-16"),
])
def test_check_fails_with_site_side_and_offsets_when_a_guard_byte_changes(fill, side, where, want_first, want_last):
    """The negative control: passes only because ``check()`` raised, and named what it must name."""
    from sageattention_amd import ops
    with Fence(fill, device_ok=ANY) as f:
        keep = torch.empty(33, dtype=torch.float16)
        lse = ops._lse_alloc(torch.zeros(2, 3, 5, 8), 1, 1)         # [2, 3, 5] fp32, allocated inside the package
        f.check()
        r = _rec(f, lse)
        base = r.lo + (r.nbytes if side == "above" else 0)
        for w in where:
            r.arena[base + w] = fill ^ 0x01
        with pytest.raises(FenceViolation) as ei:
            f.check()
        msg = str(ei.value)
        assert re.search(r"allocated at sageattention_amd/ops\.py:\d+", msg), msg
        assert "(2, 3, 5) float32" in msg and f"{len(where)} guard byte(s) {side} the buffer" in msg, msg
        assert f"first at {want_first}, last at {want_last}" in msg, msg
        assert "float16" not in msg and ("below" if side == "above" else "above") not in msg, "the untouched arena and side are not blamed"
        for w in where:
            r.arena[base + w] = fill
        f.check()
        del keep


@pytest.mark.parametrize("layout", ["HND", "NHD"])
def test_inputs_with_gap_rows_are_views_whose_gap_is_checked(layout):
    g = torch.Generator().manual_seed(0)
    shape = (2, 3, 37, 40) if layout == "HND" else (2, 37, 3, 40)
    src = torch.randn(shape, generator=g).half()
    with Fence(0xFF, device_ok=ANY) as f:
        plain = fence.fenced_input(f, src, device="cpu")
        assert torch.equal(plain, src) and plain.is_contiguous() and f.owns(plain) and plain.data_ptr() != src.data_ptr()
        t = f.input(src, gap_rows=8, tensor_layout=layout, device="cpu")
        assert torch.equal(t, src) and t.shape == src.shape and not t.is_contiguous() and t.stride(-1) == 1 and f.owns(t)
        assert all(s % 8 == 0 for s in t.stride()[:-1]) and t.data_ptr() % 16 == 0
        seq = 2 if layout == "HND" else 1
        assert t.stride(0) == (37 + 8) * 3 * 40                     # gap rows behind every head, not only the last one
        r = _rec(f, t)
        assert r.gap.shape[seq] == 8 and bool(r.gap.isnan().all())
        f.check()
        t.fill_(2.0)                                                # owned rows only
        f.check()
        row = t.select(seq, 36)                                     # the last owned row of every head ...
        row.as_strided(row.shape, row.stride(), row.storage_offset() + t.stride(seq))[1, 2, 7] = 1.0   # ... and one element one row further
        with pytest.raises(FenceViolation, match=r"caller tensor with gap rows \(2, (3, 37|37, 3), 40\) float16 allocated at test_fence_host\.py:\d+: "
                                                 r"2 byte\(s\) of the gap rows changed"):
            f.check()
        o = f.output(shape, torch.bfloat16, gap_rows=8, tensor_layout=layout, device="cpu")
        assert o.shape == shape and bool(o.isnan().all())


def test_non_contiguous_inputs_keep_their_strides():
    src = torch.arange(2 * 5 * 3 * 8, dtype=torch.float32).view(2, 5, 3, 8).transpose(1, 2)
    with Fence(0x5A, device_ok=ANY) as f:
        t = f.input(src, device="cpu")
        assert torch.equal(t, src) and t.stride() == src.stride() and f.owns(t)
        f.check()


def test_allocation_functions_are_restored_also_when_the_body_raises():
    from sageattention_amd import _stream_cache
    before = (torch.empty, torch.zeros, torch.empty_like)
    with Fence(0xFF, device_ok=ANY) as f:
        assert torch.empty is not before[0] and torch.zeros is not before[1] and torch.empty_like is not before[2]
    assert (torch.empty, torch.zeros, torch.empty_like) == before and f.arenas == []
    _stream_cache._CACHE[("attn_tickets", 0, 0)] = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="boom"):
        with Fence(0x5A, device_ok=ANY) as f:
            assert not _stream_cache._CACHE, "cached ticket / pre-pass blocks are dropped on entry: they are re-created under the fence"
            _stream_cache._CACHE[("attn_tickets", 0, 0)] = torch.zeros(4, dtype=torch.int32)
            raise RuntimeError("boom")
    assert (torch.empty, torch.zeros, torch.empty_like) == before
    assert not _stream_cache._CACHE, "no fenced block outlives the context"
    assert torch.empty(3).shape == (3,)
