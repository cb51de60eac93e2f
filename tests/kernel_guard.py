"""Guard bands around kernel operands: ``[guard | interior | guard]`` in ONE allocation.

The kernels work on tiles and cover the edges of their problem with store masks, tap masks or
buffer resources.  A fresh allocation hides a wrong mask: a store one tile row past ``M`` lands in
allocator slack, a read past the last image returns whatever the allocator left there.  A tensor
from :func:`guarded` sits between two guards the test owns:

* both guards (and, for an output, the interior) hold NaN — bf16 ``0x7FC0``, the fp32 quiet NaN,
  ``0xA5`` bytes for integer types — so an out-of-tensor read that reaches an accumulator makes
  the output non-finite.  ``0xA5`` is a finite number when a 1-byte tensor stores fp8 values or
  E8M0 block scales: ``guarded(..., poison=0xFF)`` fills such a tensor with ``0xFF`` instead, which
  is NaN both as e4m3fn and as an E8M0 scale;
* ``check()`` compares both guards bit for bit against a saved copy, so an out-of-tensor store
  is reported with its side and first offset.

Each guard holds at least ``max(numel of one image, 256 rows x row pitch)`` elements (an image is
``shape[1:]``, a row is ``shape[-1]``), rounded up to 256 bytes: an overrun of one full tile lands
in memory the test owns (for a 1-D tensor a guard is as long as the tensor, at least 256
elements).  Two things are NOT detected here:

* an overrun that jumps further than one guard;
* an out-of-tensor tap of a max-reduction: ``fmaxf`` drops a NaN operand, so max-pool kernels
  (maxpool, sppf_pool, the pooling stage of stem_pool) stay finite — and bit-identical to a run
  on fresh tensors whenever the real window maximum wins.  ``guarded(..., poison=3e38)`` fills the
  guards (and an input's poison gap channels, the caller's business) with a large finite value
  instead, which wins every maximum and so shows in the result.

A plain module (no fixtures, no device requirement): works on the CPU and on a GPU alike.
"""
from __future__ import annotations

import math

import torch

ALIGN = 256            # bytes: the interior's data_ptr() alignment (and the guard granule)
TILE_ROWS = 256        # the tallest M tile of any kernel in the project
INT_POISON = 0xA5

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class GuardError(AssertionError):
    """A guard changed: ``side`` is "before" or "after"; ``offset`` counts elements from the
    interior (before: -1 is the element just in front of it; after: 0 is the one just past it)."""

    def __init__(self, side: str, offset: int, name: str = ""):
        self.side, self.offset = side, offset
        where = f"{-offset} element(s) before the tensor" if side == "before" else \
            f"{offset} element(s) past the tensor's end"
        super().__init__(f"guard {side} {name or 'tensor'} changed: first difference {where}")


BYTE_NAN = 0xFF        # NaN as e4m3fn (S.1111.111) and as an E8M0 scale: the poison of fp8 storage


def _poison_(flat: torch.Tensor, poison=None) -> None:
    if flat.dtype.is_floating_point:
        flat.fill_(float("nan") if poison is None else poison)
    else:
        flat.view(torch.uint8).fill_(INT_POISON if poison is None else poison)


def guard_elems(shape, dtype) -> int:
    """Elements per guard for a tensor of ``shape`` / ``dtype`` (see the module docstring)."""
    shape = tuple(int(s) for s in shape)
    item = torch.empty(0, dtype=dtype).element_size()
    if len(shape) > 1:
        n = max(math.prod(shape[1:]), TILE_ROWS * shape[-1], 1)
    else:                                # 1-D: no row pitch to multiply, the whole tensor is the "image"
        n = max(math.prod(shape), TILE_ROWS)
    return (n * item + ALIGN - 1) // ALIGN * ALIGN // item


def guarded(shape, dtype, device="cpu", fill=None, values=None, name: str = "", poison=None):
    """Allocate ``[guard | interior | guard]`` and return ``(view, check)``.

    ``view`` is the interior reshaped to ``shape``: contiguous, at a non-zero storage offset and
    with a 256-byte aligned ``data_ptr()`` (alignment-selected kernel paths stay those of a fresh
    allocation).  The interior is copied from ``values`` (an input), filled with ``fill``, or —
    by default — poisoned like the guards (an output: "every element written" is
    ``isfinite(view).all()``).  ``check()`` raises :class:`GuardError` if either guard differs
    from its saved copy.  ``poison``: a finite value for the guards of a floating-point tensor
    instead of NaN (max-reductions, see the module docstring); an output's interior stays NaN.
    For a 1-byte tensor ``poison`` is a byte value (``BYTE_NAN`` for fp8 / E8M0 storage) that
    replaces ``0xA5`` in the guards and in an output's interior.
    ``check.flat`` / ``check.start`` / ``check.numel`` give the whole buffer and the interior's
    element range in it (tests extend a view into a guard with them).
    """
    shape = tuple(int(s) for s in shape)
    item = torch.empty(0, dtype=dtype).element_size()
    n = math.prod(shape)
    if poison is not None and not dtype.is_floating_point:
        if item != 1 or int(poison) != poison or not 0 <= poison <= 0xFF:
            raise ValueError(f"guarded: poison {poison!r} for {dtype}: a byte value for a 1-byte tensor only")
        poison = int(poison)
    g = guard_elems(shape, dtype)
    flat = torch.empty(2 * g + n + ALIGN // item, dtype=dtype, device=device)
    lead = (-flat.data_ptr()) % ALIGN
    assert lead % item == 0
    start = lead // item + g
    _poison_(flat, poison)
    view = flat[start:start + n].view(shape)
    if values is not None:
        view.copy_(values.to(dtype).reshape(shape))
    elif fill is not None:
        view.fill_(fill)
    elif poison is not None and dtype.is_floating_point:
        _poison_(view)
    assert view.is_contiguous() and view.storage_offset() > 0 and view.data_ptr() % ALIGN == 0
    iv = _INT_VIEW[item]
    before, after = flat[:start].view(iv), flat[start + n:].view(iv)
    saved = (before.clone(), after.clone())

    def check() -> None:
        for side, now, ref in (("before", before, saved[0]), ("after", after, saved[1])):
            if not torch.equal(now, ref):
                first = int(torch.nonzero(now != ref)[0].item())
                raise GuardError(side, first - start if side == "before" else first, name)

    check.flat, check.start, check.numel, check.name = flat, start, n, name
    return view, check
