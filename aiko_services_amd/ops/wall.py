"""Camera wall (``csrc/kernels/wall_ops.hip``): B uint8 frames (batch row ``b`` is camera ``b``)
reduced to P pages of ``rows`` x ``cols`` tiles in one picture, each tile numbered, the tiles where
something happens ringed or moved to the front.  Which camera a tile shows is decided on the
device from an int32 ``score`` per camera (the detector's ``counts``, the motion detector's
``motion_cells``): two launches, ``wall_select`` and ``wall_compose``, no host copy, no
synchronisation, hipGraph-capturable.  The wall is an ordinary uint8 ``[P, Hw, Ww, 3]`` batch that
``JpegEncode``, ``RgbToYuv`` and ``FrameDownload`` take as it is.

The rule (kernel and ``ops.reference.frame_wall_ref`` both follow it; all arithmetic is integer, so
they agree bit for bit):

* **Selection.**  With ``order="index"`` the list is 0, 1, ..., B-1.  With ``order="score"``
  (``score`` required, B <= 4096) it is the cameras with ``score[b] >= min_score`` by score
  descending, ties to the lower index.  Let M be its length and N = ``rows * cols``.  Slot
  ``j = p*N + t`` shows ``list[j]`` if ``j < M``; otherwise it is empty and ``source[p, t] = -1``.
  Frames of cameras that are not shown are never read.
* **Layout.**  Tile ``t`` sits at row ``t // cols`` and column ``t % cols``; with tile = (th, tw) and
  gap g its origin is ``(g + r*(th+g), g + c*(tw+g))``, so the wall is ``Hw = rows*th + (rows+1)*g``
  by ``Ww = cols*tw + (cols+1)*g``.  Every pixel outside a shown tile is ``background``.
* **Content.**  The exact area average with one rounding.  Source column ``j`` weighs
  ``wx(j, x) = max(0, min((j+1)*W, (x+1)*tw) - max(j*W, x*tw))`` in output column ``x``, source row
  ``i`` weighs ``wy(i, y)`` likewise with H and th; the weights of an output pixel sum to ``W*H``.
  Per channel ``S = sum wy*wx*p`` and the result is ``(2*S + W*H) // (2*W*H)``.  ``H*W <= 2**23``
  is required: then ``S <= 255 * 2**23`` and ``2*S + W*H <= 511 * 2**23 < 2**32``, so the kernel's
  unsigned 32-bit sums are exact.  A tile of (H, W) is therefore a copy, and a tile that divides the
  frame by an integer f shows the redaction's cell colour for block f (``ops.redact``).  1 <= th <=
  H and 1 <= tw <= W: the wall reduces or copies, it never enlarges.
* **Ring.**  If ``score`` is given, ``score[cam] >= min_score`` and ``ring`` = q > 0, the tile's
  pixels with ``min(i, j, th-1-i, tw-1-j) < q`` become ``alert`` (0 <= 2q <= min(th, tw)).
* **Label.**  If ``label_scale`` = s > 0: the decimal digits (n of them) of ``label_base + cam`` in
  the overlay font (``ops.overlay_font``).  The box starts at tile-local (q, q), is ``s + n*6*s``
  wide and ``s + 8*s`` high and is clipped to the tile; inside it, after the s-pixel left and top
  pad, each 6 x 8 font cell is scaled by s.  A set glyph bit gives ``label_fg``, everything else in
  the box ``label_bg``.
* **Priority.**  Label over ring over content.
"""
from __future__ import annotations

import torch

__all__ = ["ORDERS", "check_parameters", "default_tile", "frame_wall", "wall_shape"]

ORDERS = {"index": 0, "score": 1}
MAX_TILES = 1024          # per page
MAX_GAP = 64
MAX_LABEL_SCALE = 4
MAX_PIXELS = 1 << 23      # H * W of a frame: the kernel's 32-bit sums
MAX_RANKED = 4096         # cameras in score order


def _integer(name, v):
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"frame_wall: {name} must be an integer, got {v!r}")
    return int(v)


def _colour(name, v):
    v = tuple(v)
    if len(v) != 3 or any(isinstance(c, bool) or int(c) != c or not 0 <= int(c) <= 255 for c in v):
        raise ValueError(f"frame_wall: {name} = three integers 0..255 (R, G, B) required, got {v!r}")
    r, g, b = (int(c) for c in v)
    return r | g << 8 | b << 16


def wall_shape(rows: int, cols: int, tile, gap: int = 0):
    """(Hw, Ww) of a wall of ``rows`` x ``cols`` tiles of ``tile`` = (th, tw) with ``gap`` pixels
    between tiles and around the grid."""
    th, tw = (int(v) for v in tile)
    return int(rows) * th + (int(rows) + 1) * int(gap), int(cols) * tw + (int(cols) + 1) * int(gap)


def default_tile(height: int, width: int, rows: int, cols: int):
    """(H // d, W // d) with d = max(rows, cols): a square grid of such tiles is about the size of
    one frame."""
    d = max(int(rows), int(cols))
    return max(int(height) // d, 1), max(int(width) // d, 1)


def check_parameters(*, rows, cols, tile, gap=0, pages=1, order="index", min_score=1, ring=0, label_scale=0,
                     label_base=0, background=(0, 0, 0), alert=(255, 0, 0), label_fg=(255, 255, 255),
                     label_bg=(0, 0, 0), frame=None):
    """Raises ``ValueError`` for parameters outside the rule's ranges (``frame`` = (H, W), where
    known, bounds the tile) and returns them as the operator takes them: a dict of integers, the
    colours packed R | G << 8 | B << 16."""
    rows, cols, gap, pages = (_integer(n, v) for n, v in (("rows", rows), ("cols", cols), ("gap", gap),
                                                          ("pages", pages)))
    tile = tuple(tile)
    if len(tile) != 2:
        raise ValueError(f"frame_wall: tile = (th, tw) required, got {tile!r}")
    th, tw = _integer("tile", tile[0]), _integer("tile", tile[1])
    if rows < 1 or cols < 1 or rows * cols > MAX_TILES:
        raise ValueError(f"frame_wall: rows, cols >= 1 and rows * cols <= {MAX_TILES} required, got {rows} x {cols}")
    if th < 1 or tw < 1:
        raise ValueError(f"frame_wall: a tile of at least 1 x 1 required, got {th} x {tw}")
    if frame is not None:
        H, W = int(frame[0]), int(frame[1])
        if th > H or tw > W:
            raise ValueError(f"frame_wall: a tile of {th} x {tw} is larger than the frame, {H} x {W}: the wall "
                             "never enlarges")
        if H * W > MAX_PIXELS:
            raise ValueError(f"frame_wall: frames of {H} x {W} exceed {MAX_PIXELS} pixels")
    if not 0 <= gap <= MAX_GAP:
        raise ValueError(f"frame_wall: 0 <= gap <= {MAX_GAP} required, got {gap}")
    if pages < 1:
        raise ValueError(f"frame_wall: pages >= 1 required, got {pages}")
    if order not in ORDERS:
        raise ValueError(f"frame_wall: order one of {sorted(ORDERS)} required, got {order!r}")
    min_score = _integer("min_score", min_score)
    if not -2 ** 31 <= min_score < 2 ** 31:
        raise ValueError(f"frame_wall: min_score must fit int32, got {min_score}")
    ring = _integer("ring", ring)
    if ring < 0 or 2 * ring > min(th, tw):
        raise ValueError(f"frame_wall: 0 <= 2 * ring <= min(tile) = {min(th, tw)} required, got ring {ring}")
    label_scale = _integer("label_scale", label_scale)
    if not 0 <= label_scale <= MAX_LABEL_SCALE:
        raise ValueError(f"frame_wall: 0 <= label_scale <= {MAX_LABEL_SCALE} required, got {label_scale}")
    label_base = _integer("label_base", label_base)
    if not 0 <= label_base < 2 ** 31:
        raise ValueError(f"frame_wall: 0 <= label_base < 2^31 required, got {label_base}")
    return dict(rows=rows, cols=cols, tile_h=th, tile_w=tw, gap=gap, pages=pages, order=ORDERS[order],
                min_score=min_score, ring=ring, label_scale=label_scale, label_base=label_base,
                background=_colour("background", background), alert=_colour("alert", alert),
                label_fg=_colour("label_fg", label_fg), label_bg=_colour("label_bg", label_bg))


def frame_wall(frames: torch.Tensor, score: torch.Tensor | None = None, *, rows: int, cols: int, tile=None,
               gap: int = 0, pages: int = 1, order: str = "index", min_score: int = 1, ring: int = 0,
               label_scale: int = 0, label_base: int = 0, background=(0, 0, 0), alert=(255, 0, 0),
               label_fg=(255, 255, 255), label_bg=(0, 0, 0), out: torch.Tensor | None = None,
               source: torch.Tensor | None = None, passes: int = 3):
    """uint8 ``[B, H, W, 3]`` frames and, optionally, int32 ``[B]`` ``score`` -> ``(wall, source)``:
    uint8 ``[pages, Hw, Ww, 3]`` (:func:`wall_shape`) and int32 ``[pages, rows*cols]``, the camera
    of every tile or -1 (the rule: this module's docstring).  ``tile`` defaults to
    :func:`default_tile`.  ``out`` / ``source`` are written if given (``pages`` is then ``out``'s)
    and may not overlap the inputs.  ``passes``: 3, or 1 / 2 to launch the selection or the
    composition alone (measurements)."""
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
        raise ValueError("frame_wall: frames uint8 [B, H, W, 3] required")
    H, W = int(frames.shape[1]), int(frames.shape[2])
    if tile is None:
        tile = default_tile(H, W, rows, cols)
    if order == "score" and score is None:
        raise ValueError("frame_wall: order 'score' requires a score")
    p = check_parameters(rows=rows, cols=cols, tile=tile, gap=gap, pages=pages if out is None else 1, order=order,
                         min_score=min_score, ring=ring, label_scale=label_scale, label_base=label_base,
                         background=background, alert=alert, label_fg=label_fg, label_bg=label_bg, frame=(H, W))
    Hw, Ww = wall_shape(p["rows"], p["cols"], (p["tile_h"], p["tile_w"]), p["gap"])
    if out is None:
        out = torch.empty(p["pages"], Hw, Ww, 3, dtype=torch.uint8, device=frames.device)
    if source is None:
        source = torch.empty(out.shape[0] if out.dim() == 4 else 0, p["rows"] * p["cols"], dtype=torch.int32,
                             device=frames.device)
    torch.ops.aiko.frame_wall_out(frames, score, p["rows"], p["cols"], p["tile_h"], p["tile_w"], p["gap"], p["order"],
                                  p["min_score"], p["ring"], p["label_scale"], p["label_base"], p["background"],
                                  p["alert"], p["label_fg"], p["label_bg"], int(passes), out, source)
    return out, source
