"""Motion detection (``csrc/kernels/motion_ops.hip``): did anything change in a fixed camera's view,
and where?  Batch row ``b`` is one camera; its background model is a :class:`MotionState` in HBM,
read and rewritten once per frame.  The moving regions come out in the detector's own row format
(``det`` ``[B, max_det, 6]`` + ``count`` ``[B]``), so the tracker, the overlay, the redaction and the
ROI crop work behind it unchanged.  Two launches, no host copy, no synchronisation,
hipGraph-capturable like :func:`~aiko_services_amd.ops.track.track_detections`.

The rule, per row and step.  It is all integer except one fp64 division, so
:func:`~aiko_services_amd.ops.reference.motion_detect_ref` (the same in plain loops) equals the
kernels bit for bit.

1. **Luma.**  ``Y = (77*R + 150*G + 29*B + 128) >> 8``; the coefficients sum to 256, so ``Y`` is in
   0..255.
2. **Grid.**  Cells of ``cell`` x ``cell`` pixels (8, 16 or 32) anchored at the frame's origin (the
   mosaic's grid of ``ops.redact``): ``Gh = ceil(H / cell)``, ``Gw = ceil(W / cell)``, the cells at
   the right and bottom edges partial.  ``Gh <= 255``, ``Gw <= 255`` and ``Gh * Gw <= 16384``:
   1080p at cell 16 (8160 cells) and 480 x 640 at cell 8 pass, 1080p at cell 8 is refused.
3. **Cell level.**  ``cur = (32*S + n) // (2*n)``, ``S`` the luma sum over the cell's ``n``
   in-frame pixels: the mean in sixteenths, rounded half up, 0..4080.
4. **Moving.**  ``s = max(seen[b], 0)``.  A cell is moving iff ``s >= warmup`` and ``|cur - bg| >
   16 * threshold``.
5. **Background.**  If ``s == 0``: ``bg' = cur``.  Else, if the cell is moving and ``learn_moving``
   is false: ``bg' = bg``.  Else ``bg' = bg + ((cur - bg + half) >> learn_shift)``, the shift
   arithmetic (floor), ``half = 1 << (learn_shift - 1)`` (0 at ``learn_shift`` 0).  ``seen' = min(s +
   1, 2^31 - 1)``.  The background stalls within half a luma level of its target (from 0 towards
   3200 at shift 4 it ends at 3193): that is the rule, not an error.
6. **Regions.**  The 8-connected components of the moving cells.  A component's label is the
   smallest raster index ``gy * Gw + gx`` among its cells, its area its cell count, its box in cells
   ``[cx0..cx1] x [cy0..cy1]``.
7. **Rows.**  The components of ``area >= min_cells`` in order of area, largest first, ties to the
   lower label; the first ``max_det`` become rows: ``x1 = cx0 * cell``, ``y1 = cy0 * cell``, ``x2 =
   min((cx1 + 1) * cell, W)``, ``y2 = min((cy1 + 1) * cell, H)``, ``score = (float)((double)area /
   (double)((cx1 - cx0 + 1) * (cy1 - cy0 + 1)))`` (the fill ratio: one fp64 division, one rounding
   to fp32), ``class = 0``.  ``count[b]`` is the number of rows written; rows at or past it are
   zeros.  At margin 0 the rect of such a row (``roi_crop``'s) is exactly the pixels of its cells.
8. **Also written.**  ``mask`` uint8 ``[B, Gh, Gw]``, 1 where a cell is moving, and ``cells`` int32
   ``[B]``, the number of moving cells before ``min_cells``.  Every element of every output is
   written.

The empty state is all zeros.  A row whose ``seen`` is not positive takes the frame as its
background whatever ``bg`` holds.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

__all__ = ["CELLS", "MotionState", "grid_shape", "motion_detect", "new_state"]

CELLS = (8, 16, 32)


class MotionState(NamedTuple):
    """``bg`` int32 ``[B, Gh, Gw]``: the background's cell levels in sixteenths of a luma level;
    ``seen`` int32 ``[B]``: frames taken in so far."""
    bg: torch.Tensor
    seen: torch.Tensor


def grid_shape(H: int, W: int, cell: int) -> tuple[int, int]:
    """``(Gh, Gw)`` of an ``H`` x ``W`` frame at ``cell``."""
    if isinstance(cell, bool) or cell not in CELLS:
        raise ValueError(f"motion: cell one of {CELLS} required, got {cell!r}")
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f"motion: H, W >= 1 required, got {H}, {W}")
    return -(-int(H) // cell), -(-int(W) // cell)


def new_state(B: int, H: int, W: int, cell: int = 16, device="cuda") -> MotionState:
    """The empty state of ``B`` cameras of ``H`` x ``W`` pixels: zeros."""
    gh, gw = grid_shape(H, W, cell)
    return MotionState(torch.zeros(B, gh, gw, dtype=torch.int32, device=device),
                       torch.zeros(B, dtype=torch.int32, device=device))


def check_parameters(cell, threshold, learn_shift, warmup, min_cells, max_det) -> None:
    """The value ranges of the rule's parameters, as ``ValueError``."""
    if isinstance(cell, bool) or cell not in CELLS:
        raise ValueError(f"motion_detect: cell one of {CELLS} required, got {cell!r}")
    for name, v, lo, hi in (("threshold", threshold, 0, 255), ("learn_shift", learn_shift, 0, 8),
                            ("warmup", warmup, 1, 2 ** 31 - 1), ("min_cells", min_cells, 1, 2 ** 31 - 1),
                            ("max_det", max_det, 1, 64)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"motion_detect: {name} an integer in {lo}..{hi} required, got {v!r}")


def motion_detect(frames: torch.Tensor, state: MotionState, *, cell: int = 16, threshold: int = 12,
                  learn_shift: int = 4, learn_moving: bool = True, warmup: int = 1, min_cells: int = 2,
                  max_det: int = 16, state_out: MotionState | None = None, det: torch.Tensor | None = None,
                  count: torch.Tensor | None = None, mask: torch.Tensor | None = None,
                  cells: torch.Tensor | None = None):
    """One step: uint8 ``[B, H, W, 3]`` ``frames`` and ``state`` -> ``(det, count, mask, cells,
    state_out)`` (the rule: this module's docstring).  ``state`` is only read; ``state_out`` (new by
    default) must be another allocation.  Parameters out of range are a ``ValueError``; shapes,
    dtypes, devices, overlap and a grid past the limits are refused by the operator."""
    check_parameters(cell, threshold, learn_shift, warmup, min_cells, max_det)
    if frames.dim() != 4:
        raise ValueError(f"motion_detect: frames [B, H, W, 3] required, got {tuple(frames.shape)}")
    B, H, W = frames.shape[:3]
    gh, gw = grid_shape(H, W, cell)
    dev = frames.device
    if state_out is None:
        state_out = MotionState(torch.empty(B, gh, gw, dtype=torch.int32, device=dev),
                                torch.empty(B, dtype=torch.int32, device=dev))
    if det is None:
        det = torch.empty(B, int(max_det), 6, dtype=torch.float32, device=dev)
    elif det.dim() != 3 or det.shape[1] != int(max_det):
        raise ValueError(f"motion_detect: det [B, max_det = {max_det}, 6] required, got {tuple(det.shape)}")
    count, cells = (torch.empty(B, dtype=torch.int32, device=dev) if t is None else t for t in (count, cells))
    if mask is None:
        mask = torch.empty(B, gh, gw, dtype=torch.uint8, device=dev)
    torch.ops.aiko.motion_detect_out(frames, state.bg, state.seen, int(cell), int(threshold), int(learn_shift),
                                     bool(learn_moving), int(warmup), int(min_cells), state_out.bg, state_out.seen,
                                     det, count, mask, cells)
    return det, count, mask, cells, state_out
