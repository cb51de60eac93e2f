"""Detection redaction (``csrc/kernels/redact_ops.hip``): the pixels inside the detector's boxes
replaced by a mosaic or a flat colour in the uint8 frames on the device, before a frame leaves it.
Rows and counts are read by the kernel: no host copy, no synchronisation, hipGraph-capturable like
:func:`~aiko_services_amd.ops.overlay.draw_detections`.

The rule (kernel and ``ops.reference.redact_detections_ref`` both follow it):

* **Used rows.**  Row ``i`` of frame ``b`` is used iff ``i < min(max(count[b], 0), k)`` and its four
  coordinates are finite (the rule of ``roi_crop``).  Rows at or past that bound are never read,
  nor are the ``labels`` of unused slots.
* **Class and selection.**  The row's class is ``labels[b*k + i]`` when ``labels`` (int32
  ``[B*k]``) is given, otherwise ``(int)det[b, i, 5]`` with NaN -> 0 and saturation: the class
  ``draw_detections`` shows.  A used row is selected iff ``select`` is None, or ``0 <= class < C and
  select[class] != 0`` (``select``: uint8 ``[C]``, ``C >= 1``; :func:`class_select` builds it).
* **Covered pixels.**  A pixel is covered iff it lies in the rect of at least one selected row; the
  rect is that of ``roi_rect.h`` / ``roi_rects_ref`` for the same ``margin``, so redaction covers
  exactly the pixels ``roi_crop`` would crop and ``draw_detections`` would outline.  Uncovered
  pixels are copied unchanged.
* **Mode** ``fill``: a covered pixel becomes ``fill``.
* **Mode** ``pixelate``: the frame carries a grid of ``block`` x ``block`` cells anchored at the
  frame's origin; cells at the right and bottom edges are partial.  A cell's colour per channel is
  ``(2*S + n) // (2*n)``, ``S`` the integer sum of that channel over the cell's ``n`` in-frame
  pixels, covered or not: all-integer, rounding half up.  A covered pixel becomes its cell's colour.
  The grid is anchored to the frame, not to the box: a box that moves a pixel does not make the
  mosaic shimmer, and overlapping boxes agree.
* **Block size.**  ``block`` is one of {4, 8, 16, 32}.  These divide both sides of the kernel's 128 x 32
  tile, so no cell straddles two workgroups and a workgroup reads all of its cells before it writes
  any: pixelation in place is safe.  (A box blur or a Gaussian would need reads across tiles and
  would not be; neither is offered.)
"""
from __future__ import annotations

import torch

__all__ = ["BLOCKS", "MODES", "class_select", "redact_detections"]

MODES = {"pixelate": 0, "fill": 1}
BLOCKS = (4, 8, 16, 32)


def class_select(classes, n: int) -> torch.Tensor:
    """Class ids -> the uint8 ``[n]`` table the kernel reads: 1 at every listed id, 0 elsewhere.
    Every id must be an integer in ``[0, n)``; an empty list selects nothing."""
    n = int(n)
    if n < 1:
        raise ValueError(f"class_select: n >= 1 required, got {n}")
    table = torch.zeros(n, dtype=torch.uint8)
    for c in classes:
        if isinstance(c, bool) or int(c) != c:
            raise ValueError(f"class_select: integer class ids required, got {c!r}")
        if not 0 <= int(c) < n:
            raise ValueError(f"class_select: class {c} outside [0, {n})")
        table[int(c)] = 1
    return table


def redact_detections(frames: torch.Tensor, det: torch.Tensor, count: torch.Tensor, k: int, *,
                      mode: str = "pixelate", block: int = 16, fill=(0, 0, 0), margin: float = 0.0,
                      select: torch.Tensor | None = None, labels: torch.Tensor | None = None,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 ``[B, H, W, 3]`` frames + ``det`` ``[B, max_det, 6]`` / ``count`` ``[B]`` (the outputs
    of :func:`~aiko_services_amd.ops.detect.topk_nms`) -> ``out``: the frames with the pixels of
    every selected row's rect pixelated or filled (the rule: this module's docstring).
    ``1 <= k <= max_det``.  ``out`` may be ``frames`` itself (redacted in place); by default it is
    new; any other overlap is refused."""
    if mode not in MODES:
        raise ValueError(f"redact_detections: mode one of {sorted(MODES)} required, got {mode!r}")
    fill = tuple(fill)
    if len(fill) != 3 or any(isinstance(c, bool) or int(c) != c for c in fill):
        raise ValueError(f"redact_detections: fill = three integers (R, G, B) required, got {fill!r}")
    r, g, b = (int(c) for c in fill)
    # a component outside 0..255 has no packed form: refused by the operator, with the other operands
    fill_rgb = r | g << 8 | b << 16 if all(0 <= c <= 255 for c in (r, g, b)) else -1
    if out is None:
        out = torch.empty_like(frames)
    torch.ops.aiko.redact_detections_out(frames, det, count, int(k), labels, select, MODES[mode], int(block),
                                         fill_rgb, float(margin), out)
    return out
