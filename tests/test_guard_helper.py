"""The guard-band helper (tests/kernel_guard.py) on the CPU: layout of the view, and that a
one-element change on either side of the interior is reported with its side and offset."""
import pytest
import torch

from kernel_guard import ALIGN, GuardError, guard_elems, guarded

DTYPES = [torch.bfloat16, torch.float32, torch.uint8]
SHAPES = [(2, 9, 11, 24), (37, 1000), (3, 5, 7, 3), (5,)]


@pytest.mark.parametrize("dtype", DTYPES + [torch.int32])
@pytest.mark.parametrize("shape", SHAPES)
def test_view_is_contiguous_offset_and_aligned(shape, dtype):
    view, check = guarded(shape, dtype)
    assert tuple(view.shape) == shape and view.dtype == dtype
    assert view.is_contiguous()
    assert view.storage_offset() > 0
    assert view.data_ptr() % ALIGN == 0
    g = guard_elems(shape, dtype)
    image = view[0].numel() if view.dim() > 1 else view.numel()
    assert g >= (max(image, 256 * shape[-1]) if view.dim() > 1 else max(view.numel(), 256))
    assert g * view.element_size() % ALIGN == 0
    assert check.start >= g and check.flat.numel() - check.start - check.numel >= g
    check()                                                    # untouched: passes


@pytest.mark.parametrize("dtype", DTYPES)
def test_contents(dtype):
    vals = torch.arange(2 * 3 * 4 * 8).reshape(2, 3, 4, 8).to(dtype)
    view, check = guarded(vals.shape, dtype, values=vals)
    assert torch.equal(view, vals)
    flat, s, n = check.flat, check.start, check.numel
    outside = torch.cat([flat[:s], flat[s + n:]])
    if dtype.is_floating_point:
        assert torch.isnan(outside.float()).all()
        bits = outside.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)
        want = 0x7FC0 if dtype == torch.bfloat16 else 0x7FC00000
        assert (bits == want).all()
        out, _ = guarded((2, 3, 4, 8), dtype)                  # an output: poisoned interior
        assert torch.isnan(out.float()).all()
    else:
        assert (outside == 0xA5).all()
        out, _ = guarded((2, 3, 4, 8), dtype)
        assert (out == 0xA5).all()
    filled, _ = guarded((2, 3), dtype, fill=7)
    assert (filled == 7).all()
    check()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side,offset", [("before", -1), ("after", 0), ("before", -300), ("before", "far"),
                                         ("after", "far")])
def test_one_element_change_is_reported(dtype, side, offset):
    vals = torch.ones(2, 5, 7, 16)
    view, check = guarded(vals.shape, dtype, values=vals, name="x")
    flat, s, n = check.flat, check.start, check.numel
    if offset == "far":                                        # the guard's outermost element
        g = guard_elems(vals.shape, dtype)
        offset = -g if side == "before" else g - 1
    at = s + offset if side == "before" else s + n + offset
    flat[at] = 3                                               # NaN / 0xA5 -> 3: one element
    with pytest.raises(GuardError) as e:
        check()
    assert e.value.side == side and e.value.offset == offset
    assert side in str(e.value) and "x" in str(e.value)
    assert torch.equal(view, vals.to(dtype))                   # the interior is not part of the check


@pytest.mark.parametrize("dtype", DTYPES)
def test_interior_writes_and_rewritten_poison_pass(dtype):
    view, check = guarded((3, 4, 8), dtype)
    view.fill_(1)
    check()
    # another NaN is still a change: the comparison is bit for bit
    if dtype.is_floating_point:
        bits = check.flat.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)
        bits[check.start - 1] |= 1
        with pytest.raises(GuardError):
            check()


def test_one_dimensional_guard_is_not_multiplied_by_its_length():
    n = 4 * 37 * 1000                                          # a split-K work buffer
    assert n <= guard_elems((n,), torch.float32) < n + 64
    assert guard_elems((5,), torch.float32) == 256
    view, check = guarded((n,), torch.float32)
    assert check.flat.numel() < 3 * n + 256
    check()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_finite_poison_for_max_reductions(dtype):
    vals = torch.zeros(2, 3, 4, 8)
    view, check = guarded(vals.shape, dtype, values=vals, poison=3e38)
    flat, s, n = check.flat, check.start, check.numel
    outside = torch.cat([flat[:s], flat[s + n:]]).float()
    assert torch.isfinite(outside).all() and (outside > 2.9e38).all()
    out, _ = guarded(vals.shape, dtype, poison=3e38)           # an output's interior stays NaN
    assert torch.isnan(out.float()).all()
    flat[s - 1] = 0
    with pytest.raises(GuardError):
        check()


def test_first_difference_wins():
    view, check = guarded((4, 8), torch.float32)
    check.flat[check.start - 5] = 0.0
    check.flat[check.start - 2] = 0.0
    check.flat[check.start + check.numel + 9] = 0.0
    with pytest.raises(GuardError) as e:
        check()
    assert (e.value.side, e.value.offset) == ("before", -5)
