"""Square fiducial markers (``csrc/kernels/marker_ops.hip``): find ArUco-style markers in uint8 RGB
frames ``[B, H, W, 3]`` at any rotation and under perspective, on the device.  The markers come out
as detector rows (``det`` ``[B, max_det, 6]`` + ``count`` ``[B]``, the id as the class), so the
tracker, the overlay, the redaction and the ROI crop work behind it unchanged, and as ``corners`` /
``ids`` for what wants the quad.  Three launches, no host copy, no synchronisation,
hipGraph-capturable.  The markers are those of ``examples/aruco_marker/aruco.py``: ``original``
(7 x 7 modules, ids 0..1023) and ``payload16`` (6 x 6 modules, the id is the smallest 16-bit payload
over the rotations).

The rule, per frame.  It is all integer except the score's one fp64 division, so
:func:`~aiko_services_amd.ops.reference.detect_markers_ref` (the same in plain loops) equals the
kernels bit for bit.

1. **Luma.**  ``Y = (77*R + 150*G + 29*B + 128) >> 8`` (``ops.motion``'s).
2. **Range grid.**  Blocks of 16 x 16 pixels anchored at the origin, the edge blocks partial: ``lo``,
   ``hi`` = min and max luma of a block's in-frame pixels.
3. **Dark pixels.**  For a pixel in block ``(ry, rx)``: ``m`` = min of ``lo`` and ``M`` = max of
   ``hi`` over the in-grid blocks of the 3 x 3 block neighbourhood.  The pixel is dark iff ``M - m >=
   contrast`` (1..255) and ``2*Y < m + M``.  The deep inside of a large black area has no contrast
   around it and is *not* dark: a marker's border stays connected through its edges, and the bits are
   not read from this mask (rule 7).
4. **Cells and components.**  Cells of ``cell`` x ``cell`` pixels (4, 8 or 16) anchored at the
   origin: ``Gh = ceil(H / cell)``, ``Gw = ceil(W / cell)``.  A cell is on iff it holds a dark pixel.
   Components are the 8-connected components of the on cells; a component's label is the smallest
   raster index ``gy * Gw + gx`` among its cells.  The padded grid is limited to ``(Gh + 2) * (Gw +
   2) <= 36864``: 480 x 640 at cell 4 and 1080p at cell 8 pass, 720p at cell 4 is refused.  Hence the
   quiet-zone rule: a marker is separate from other dark pixels whenever every one of them is at
   Chebyshev distance >= ``2 * cell`` from it; nearer than that they may merge and the marker is
   lost.
5. **Candidates.**  A component whose pixel box (its cell box clipped to the frame) has ``min(w, h)
   >= min_side``, in ascending label order.  The first ``max_cand`` (<= 64) are examined;
   ``cands[b]`` counts all of them.
6. **Corners.**  Over the dark pixels ``(x, y)`` in cells of the candidate's own label, eight
   extremes, each maximising a primary, ties to the lower ``y``, then the lower ``x``.  The diagonal
   quad is ``[min(x+y), max(x-y), max(x+y), min(x-y)]``, the axial quad ``[min y, max x, max y, min
   x]``: both clockwise from the top (left).  The quad with the larger doubled shoelace area
   ``|sum(x_i * y_(i+1) - x_(i+1) * y_i)|`` is taken, the diagonal one on a tie.
7. **Sampling.**  ``N`` = 7 (``original``) or 6 (``payload16``).  The quad ``C0..C3`` is the image
   of the unit square under a projective map, in exact integers: ``dx1 = x1-x2``, ``dx2 = x3-x2``,
   ``sx = x0-x1+x2-x3`` (likewise in ``y``), ``den = dx1*dy2 - dy1*dx2``, ``G = sx*dy2 - sy*dx2``,
   ``Hh = dx1*sy - dy1*sx``, ``A = den*(x1-x0) + G*x1``, ``Bx = den*(x3-x0) + Hh*x3``, ``D =
   den*(y1-y0) + G*y1``, ``E = den*(y3-y0) + Hh*y3``.  Module ``(i, j)`` (row, column) with ``a =
   2j+1``, ``b = 2i+1``: ``dd = G*a + Hh*b + 2N*den``, ``nx = A*a + Bx*b + 2N*den*x0``, ``ny = D*a
   + E*b + 2N*den*y0``, all three negated if ``dd < 0``; ``px = floor((2*nx + dd) / (2*dd))``,
   likewise ``py``, clamped into the frame.  Every intermediate fits int64 for ``H, W <= 4096``;
   larger frames are refused.  ``den == 0`` or any ``dd == 0`` rejects the candidate.  The sample is
   the luma of that one pixel; ``lo_s``, ``hi_s`` = min and max over the ``N*N`` samples; ``hi_s -
   lo_s < contrast`` rejects; a module is white iff ``2*Y >= lo_s + hi_s``.
8. **Decode.**  All ``4N - 4`` border modules must be black.  The inner bits are decoded as
   ``examples/aruco_marker/aruco.py`` decodes them, over the rotations ``np.rot90(bits, -r)``, ``r =
   0..3``: ``original`` takes the first ``r`` for which ``decode_original`` gives an id,
   ``payload16`` the smallest ``_code`` and its first ``r``.  The corners are rolled as there
   (``quad[(i + (4 - r) % 4) % 4]``), the marker's own top-left first.  No rotation decoding
   rejects the candidate.
9. **Outputs.**  The accepted candidates in candidate order, the first ``max_det`` (<= 64) of them:
   ``corners`` int32 ``[B, max_det, 4, 2]`` (``(x, y)`` pixel indices), ``ids`` int32 ``[B,
   max_det]`` (-1 past the count), ``det`` fp32 ``[B, max_det, 6]`` (``x1, y1`` = the corners'
   minima, ``x2, y2`` = their maxima + 1, ``score = (float)((double)(hi_s - lo_s) / 255.0)``,
   ``class = (float)id``; the rest zeros, as in ``corners``), ``count`` / ``cands`` int32 ``[B]``,
   ``mask`` uint8 ``[B, Gh, Gw]`` (the on cells).  Every element of every output is written.

``work`` is the kernels' workspace, int32 ``[work_size(B, H, W)]``: the packed dark mask ``[B, H,
ceil(W / 32)]`` and the range grid.
"""
from __future__ import annotations

import torch

__all__ = ["CELLS", "DICTIONARIES", "MAX_GRID", "MAX_SIDE", "check_parameters", "detect_markers", "dictionary_of",
           "grid_shape", "work_size"]

CELLS = (4, 8, 16)
DICTIONARIES = {"original": 7, "payload16": 6}          # modules per side, border included
MAX_GRID = 36864                                        # (Gh + 2) * (Gw + 2): 72 KB of 16-bit labels in LDS
MAX_SIDE = 4096                                         # H, W: the sampling's intermediates fit int64
BLOCK = 16                                              # pixels per side of a range block


def grid_shape(H: int, W: int, cell: int = 4) -> tuple[int, int]:
    """``(Gh, Gw)`` of an ``H`` x ``W`` frame at ``cell``."""
    if isinstance(cell, bool) or cell not in CELLS:
        raise ValueError(f"marker: cell one of {CELLS} required, got {cell!r}")
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f"marker: H, W >= 1 required, got {H}, {W}")
    return -(-int(H) // cell), -(-int(W) // cell)


def work_size(B: int, H: int, W: int) -> int:
    """int32 elements of the workspace for ``B`` frames of ``H`` x ``W``."""
    return int(B) * (int(H) * (-(-int(W) // 32)) + (-(-int(H) // BLOCK)) * (-(-int(W) // BLOCK)))


def dictionary_of(aruco_tags) -> str:
    """The dictionary of the host element's ``aruco_tags`` parameter: ``DICT_ARUCO_ORIGINAL`` is
    ``original``, every other tag ``payload16`` (``examples/aruco_marker/aruco.py``)."""
    return "original" if str(aruco_tags) == "DICT_ARUCO_ORIGINAL" else "payload16"


def check_parameters(dictionary, cell, contrast, min_side, max_cand, max_det) -> None:
    """The value ranges of the rule's parameters, as ``ValueError``."""
    if dictionary not in DICTIONARIES:
        raise ValueError(f"detect_markers: dictionary one of {tuple(DICTIONARIES)} required, got {dictionary!r}")
    if isinstance(cell, bool) or cell not in CELLS:
        raise ValueError(f"detect_markers: cell one of {CELLS} required, got {cell!r}")
    for name, v, lo, hi in (("contrast", contrast, 1, 255), ("min_side", min_side, 1, MAX_SIDE),
                            ("max_cand", max_cand, 1, 64), ("max_det", max_det, 1, 64)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"detect_markers: {name} an integer in {lo}..{hi} required, got {v!r}")


def detect_markers(frames: torch.Tensor, *, dictionary: str = "original", cell: int = 4, contrast: int = 64,
                   min_side: int = 24, max_cand: int = 32, max_det: int = 16, det: torch.Tensor | None = None,
                   count: torch.Tensor | None = None, corners: torch.Tensor | None = None,
                   ids: torch.Tensor | None = None, cands: torch.Tensor | None = None,
                   mask: torch.Tensor | None = None, work: torch.Tensor | None = None):
    """uint8 ``[B, H, W, 3]`` ``frames`` -> ``(det, count, corners, ids, cands, mask)`` (the rule:
    this module's docstring).  Parameters out of range are a ``ValueError``; shapes, dtypes, devices,
    overlap, frames above 4096 pixels a side and a grid past the limit are refused by the operator."""
    check_parameters(dictionary, cell, contrast, min_side, max_cand, max_det)
    if frames.dim() != 4:
        raise ValueError(f"detect_markers: frames [B, H, W, 3] required, got {tuple(frames.shape)}")
    B, H, W = frames.shape[:3]
    gh, gw = grid_shape(H, W, cell)
    dev = frames.device
    if det is None:
        det = torch.empty(B, int(max_det), 6, dtype=torch.float32, device=dev)
    elif det.dim() != 3 or det.shape[1] != int(max_det):
        raise ValueError(f"detect_markers: det [B, max_det = {max_det}, 6] required, got {tuple(det.shape)}")
    count, cands = (torch.empty(B, dtype=torch.int32, device=dev) if t is None else t for t in (count, cands))
    if corners is None:
        corners = torch.empty(B, int(max_det), 4, 2, dtype=torch.int32, device=dev)
    if ids is None:
        ids = torch.empty(B, int(max_det), dtype=torch.int32, device=dev)
    if mask is None:
        mask = torch.empty(B, gh, gw, dtype=torch.uint8, device=dev)
    if work is None:
        work = torch.empty(work_size(B, H, W), dtype=torch.int32, device=dev)
    torch.ops.aiko.marker_detect_out(frames, DICTIONARIES[dictionary], int(cell), int(contrast), int(min_side),
                                     int(max_cand), 7, det, count, corners, ids, cands, mask, work)
    return det, count, corners, ids, cands, mask
