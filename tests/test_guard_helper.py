"""The guard-band helper (tests/kernel_guard.py) on the CPU: layout of the view, and that a
one-element change on either side of the interior is reported with its side and offset."""
import pytest
import torch

from guard_ops import ROW_BOUND, assert_pixel_channel, pixel_channel_errs, row_err, row_errs
from kernel_guard import ALIGN, BYTE_NAN, GuardError, guard_elems, guarded

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


# ---- byte poison for fp8 / E8M0 storage -----------------------------------------------------------

def test_byte_poison_is_nan_as_e4m3_and_as_e8m0():
    assert BYTE_NAN == 0xFF
    b = torch.tensor([BYTE_NAN], dtype=torch.uint8)
    assert torch.isnan(b.view(torch.float8_e4m3fn).float()).all()          # S.1111.111
    a5 = torch.tensor([0xA5], dtype=torch.uint8)
    assert torch.isfinite(a5.view(torch.float8_e4m3fn).float()).all()      # the default poison: a number
    # E8M0 has one NaN, 0xFF (OCP MX v1.0); 0xA5 would be the scale 2^38 — torch has no such dtype
    # on every build, so this is the format's definition, not a conversion
    assert BYTE_NAN == 2 ** 8 - 1 and 0xA5 - 127 == 38


@pytest.mark.parametrize("shape", [(37, 1000), (3, 128, 4), (5,)])
def test_byte_poison_fills_guards_and_output_interior(shape):
    out, check = guarded(shape, torch.uint8, poison=BYTE_NAN)
    assert (check.flat == 0xFF).all() and (out == 0xFF).all()              # guards and interior
    assert out.is_contiguous() and out.data_ptr() % ALIGN == 0
    check()
    vals = torch.arange(out.numel()).reshape(shape) % 200
    inp, check = guarded(shape, torch.uint8, values=vals, poison=BYTE_NAN)
    flat, s, n = check.flat, check.start, check.numel
    assert torch.equal(inp, vals.to(torch.uint8))
    assert (flat[:s] == 0xFF).all() and (flat[s + n:] == 0xFF).all()
    filled, _ = guarded(shape, torch.uint8, fill=127, poison=BYTE_NAN)
    assert (filled == 127).all()
    default, c = guarded(shape, torch.uint8)                               # unchanged: 0xA5
    assert (c.flat == 0xA5).all()


@pytest.mark.parametrize("side,offset", [("before", -1), ("after", 0), ("after", 700)])
def test_byte_poison_change_is_reported(side, offset):
    view, check = guarded((3, 128, 4), torch.uint8, fill=127, poison=BYTE_NAN, name="scales")
    at = check.start + offset if side == "before" else check.start + check.numel + offset
    check.flat[at] = 0xA5                                                  # 0xFF -> the default poison
    with pytest.raises(GuardError) as e:
        check()
    assert (e.value.side, e.value.offset) == (side, offset) and "scales" in str(e.value)
    assert (view == 127).all()


@pytest.mark.parametrize("dtype,poison", [(torch.int32, 0xFF), (torch.int16, 0xFF), (torch.uint8, 256),
                                          (torch.uint8, -1), (torch.uint8, 1.5)])
def test_byte_poison_is_for_one_byte_tensors_only(dtype, poison):
    with pytest.raises(ValueError):
        guarded((4, 8), dtype, poison=poison)


# ---- the per-row metric ----------------------------------------------------------------------------

def _rel(a, b):                                     # the whole-tensor number of test_gpu_transformer.py
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def test_row_err_basics():
    ref = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1.0, 0.0]])
    assert row_err(ref.clone(), ref) == 0.0
    y = ref.clone()
    y[0, 0] = 3.5                                                          # 0.5 / 5
    assert abs(row_err(y, ref) - 0.1) < 1e-12
    y = ref.clone()
    y[1, 1] = 1e-30                                                        # a zero row is compared exactly
    assert row_err(y, ref) == float("inf")
    y = ref.clone()
    y[2, 1] = float("nan")
    assert row_err(y, ref) == float("inf")
    assert row_err(ref.to(torch.bfloat16), ref) == 0.0                     # any dtype in, fp64 inside


def test_row_err_flags_what_the_whole_tensor_norm_lets_through():
    """A GEMM output at the shape of test_gemm_fp8 (333 x 384, K = 768, weights / 30, the Whisper
    model's bias scale 0.02), rounded to bf16 as a kernel would.  One row off by 5 % and a missing
    bias on the last 5 rows (a tail the size of a partial tile) both stay under the whole-tensor
    ``_rel < 5e-3`` of the existing tests; the per-row bound 2^-8 flags both, and passes the clean
    output, whose rows carry one bf16 rounding: at most 2^-8 of an element (half an ulp of 8
    significand bits), about 2^-9 of a row's norm."""
    g = torch.Generator().manual_seed(0)
    M, N, K = 333, 384, 768
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    w = torch.randn(N, K, generator=g, dtype=torch.float64) / 30
    bias = 0.02 * torch.randn(N, generator=g, dtype=torch.float64)
    ref = x @ w.T + bias
    clean = ref.to(torch.bfloat16)
    assert ROW_BOUND == 2.0 ** -8
    assert 2.0 ** -10 < row_err(clean, ref) < 0.6 * ROW_BOUND
    scaled = clean.clone()
    scaled[200] = (ref[200] * 1.05).to(torch.bfloat16)
    assert _rel(scaled, ref) < 5e-3                                        # the old bound: passes
    assert row_err(scaled, ref) > ROW_BOUND                                # the new one: flagged
    assert 0.045 < row_err(scaled, ref) < 0.055
    nobias = clean.clone()
    nobias[M - 5:] = (ref[M - 5:] - bias).to(torch.bfloat16)
    assert _rel(nobias, ref) < 5e-3
    assert row_err(nobias, ref) > ROW_BOUND


# ---- the per-pixel / per-channel metric ------------------------------------------------------------

def _pc_ref():
    g = torch.Generator().manual_seed(3)
    return torch.randn(2, 3, 5, 8, generator=g, dtype=torch.float64) + 0.5


def test_row_errs_is_what_row_err_reduces():
    ref = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1.0, 0.0]])
    y = ref.clone()
    y[0, 0] = 3.5
    errs = row_errs(y, ref)
    assert errs.dtype == torch.float64 and errs.shape == (3,)
    assert abs(errs[0].item() - 0.1) < 1e-12 and errs[1].item() == 0.0 and errs[2].item() == 0.0
    assert row_err(y, ref) == errs.max().item()
    empty = torch.zeros(0, 4)
    assert row_errs(empty, empty).numel() == 0 and row_err(empty, empty) == 0.0


def test_pixel_channel_errs_exact_row_column_zero_norm_and_nan():
    ref = _pc_ref()
    pix, ch = pixel_channel_errs(ref.clone(), ref)
    assert pix.shape == (30,) and ch.shape == (8,) and pix.max().item() == 0.0 and ch.max().item() == 0.0
    assert_pixel_channel(ref.clone(), ref, ROW_BOUND, "exact")
    y = ref.clone()
    y[1, 2, 4] *= 1.01                                                     # one pixel row off by 1 %
    pix, ch = pixel_channel_errs(y, ref)
    assert abs(pix[29].item() - 0.01) < 1e-12 and (pix[:29] == 0).all()
    assert (ch > 0).all() and ch.max().item() < 0.01                       # one of 30 entries per column
    y = ref.clone()
    y[..., 5] *= 1.01                                                      # one channel column off by 1 %
    pix, ch = pixel_channel_errs(y, ref)
    assert abs(ch[5].item() - 0.01) < 1e-12 and ch[:5].max().item() == 0 and ch[6:].max().item() == 0
    assert (pix > 0).all() and pix.max().item() < 0.01
    zref = ref.clone()
    zref[0, 1, 3] = 0                                                      # a zero-norm pixel row: compared exactly
    pix, _ = pixel_channel_errs(zref.clone(), zref)
    assert pix.max().item() == 0.0
    y = zref.clone()
    y[0, 1, 3, 2] = 1e-30
    pix, ch = pixel_channel_errs(y, zref)
    assert pix[8].item() == float("inf") and torch.isfinite(ch).all()
    y = ref.clone()
    y[0, 0, 1, 6] = float("nan")
    pix, ch = pixel_channel_errs(y, ref)
    assert pix[1].item() == float("inf") and ch[6].item() == float("inf")
    assert torch.isfinite(pix).sum().item() == 29 and torch.isfinite(ch).sum().item() == 7
    pix2, ch2 = pixel_channel_errs(ref.reshape(30, 8).to(torch.bfloat16), ref.reshape(30, 8))   # [M, N], any dtype
    assert 0 < pix2.max().item() < ROW_BOUND and 0 < ch2.max().item() < ROW_BOUND


def test_assert_pixel_channel_names_the_pattern(capsys):
    ref = _pc_ref()
    pe, ce = assert_pixel_channel(ref.to(torch.bfloat16), ref, ROW_BOUND, "clean")
    assert 0 < pe < ROW_BOUND and 0 < ce < ROW_BOUND
    out = capsys.readouterr().out
    assert "clean" in out and "worst pixel (" in out and "worst channel" in out
    y = ref.clone()
    y[1, 0, 4] *= 1.05                                                     # right-hand column of image 1
    y[1, 2, 4] *= 1.05
    with pytest.raises(AssertionError) as e:
        assert_pixel_channel(y, ref, ROW_BOUND, "border")
    msg = str(e.value)
    assert "border" in msg and "2 of 30 pixels" in msg and "first (1, 0, 4) (row 19)" in msg
    assert "last (1, 2, 4) (row 29)" in msg
    assert "worst pixel (1," in capsys.readouterr().out                    # printed before it asserts
    y = ref.clone()
    y[..., 7] = 0                                                          # the last channel lost
    with pytest.raises(AssertionError) as e:
        assert_pixel_channel(y, ref, ROW_BOUND, "tail")
    assert "1 of 8 channels: first 7" in str(e.value) and "last 7" in str(e.value)
    y = ref.clone()
    y[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError) as e:
        assert_pixel_channel(y, ref, ROW_BOUND, "nan")
    assert "1 of 30 pixels" in str(e.value) and "1 of 8 channels" in str(e.value) and "inf" in str(e.value)
    with pytest.raises(AssertionError):
        assert_pixel_channel(ref.clone(), ref, 0.0, "zero bound")          # strictly below the bound
