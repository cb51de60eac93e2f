"""Detection overlay (``csrc/kernels/overlay_ops.hip``): the detector's fixed-size NMS rows — and
optionally a classifier's class and probability per ROI slot — drawn as boxes and labels into the
uint8 frames on the device.  Rows and counts are read by the kernel: no host copy, no
synchronisation, hipGraph-capturable like :func:`~aiko_services_amd.ops.roi.roi_crop`."""
from __future__ import annotations

import colorsys

import torch

from . import overlay_font

__all__ = ["default_font", "default_palette", "draw_detections", "pack_names"]


def pack_names(names, width: int = 16) -> torch.Tensor:
    """Class names -> the uint8 ``[C, width]`` table the kernel reads: ASCII, truncated to
    ``width`` bytes, zero-padded (a name ends at its first zero byte)."""
    if not 1 <= int(width) <= 32:
        raise ValueError(f"pack_names: 1 <= width <= 32 required, got {width}")
    table = torch.zeros(len(names), int(width), dtype=torch.uint8)
    for i, name in enumerate(names):
        raw = str(name).encode("ascii")[:width]
        table[i, :len(raw)] = torch.tensor(list(raw), dtype=torch.uint8)
    return table


def default_palette(n: int = 20) -> torch.Tensor:
    """A deterministic uint8 ``[n, 3]`` RGB table: the hue advances by the golden ratio from one
    entry to the next (neighbouring classes are far apart on the colour wheel) and three
    brightness / saturation levels rotate, so hues that come close again still differ."""
    if n < 1:
        raise ValueError("default_palette: n >= 1 required")
    levels = ((1.0, 0.90), (0.70, 1.0), (0.95, 0.55))         # (value, saturation)
    rows = []
    for i in range(n):
        v, s = levels[i % 3]
        rgb = colorsys.hsv_to_rgb((i * 0.6180339887498949) % 1.0, s, v)
        rows.append([int(round(c * 255)) for c in rgb])
    return torch.tensor(rows, dtype=torch.uint8)


def default_font() -> tuple[torch.Tensor, int]:
    """(``font`` uint8 ``[95, 8]``, ``glyph_width`` 6): the project's 5 x 7 font in its 6 x 8 cell
    (:mod:`~aiko_services_amd.ops.overlay_font`), codes 32..126."""
    return torch.tensor(overlay_font.atlas(), dtype=torch.uint8), overlay_font.CELL_W


def draw_detections(frames: torch.Tensor, det: torch.Tensor, count: torch.Tensor, k: int, names: torch.Tensor,
                    font: torch.Tensor, palette: torch.Tensor, *, labels: torch.Tensor | None = None,
                    scores: torch.Tensor | None = None, thickness: int = 2, text_scale: int = 1,
                    margin: float = 0.0, show_score: bool = True, glyph_width: int | None = None,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 ``[B, H, W, 3]`` frames + ``det`` ``[B, max_det, 6]`` / ``count`` ``[B]`` (the outputs
    of :func:`~aiko_services_amd.ops.detect.topk_nms`) -> ``out``: the frames with one box and one
    label per used row.  ``out`` may be ``frames`` itself (drawn in place); by default it is new.

    Row ``i`` of frame ``b`` is used iff ``i < min(count[b], k)`` and its coordinates are finite
    (the rule of ``roi_crop``); its rect is the one ``roi_crop`` reports for the same ``margin``.
    Slot ``b*k + i`` of ``labels`` (int32) / ``scores`` (fp32) replaces the detector's class /
    score.  The colour is ``palette[class % P]`` (``palette[0]`` for a negative class), the
    outline is ``thickness`` pixels wide inside the rect, and the label — ``names[class]``, then a
    two-digit percentage of the score if ``show_score`` — sits above the box (inside its top when
    there is no room), in black or white by the colour's luma, ``text_scale`` pixels per font
    pixel.  ``font`` is uint8 ``[G, gh]``: one byte per glyph row, bit 7 leftmost, ``glyph_width``
    columns used (default: the cell width of :func:`default_font`), glyph ``g`` = code ``32 + g``.
    Where rows overlap the lowest index (the highest score) is on top."""
    if out is None:
        out = torch.empty_like(frames)
    gw = overlay_font.CELL_W if glyph_width is None else int(glyph_width)
    torch.ops.aiko.draw_detections_out(frames, det, count, int(k), labels, scores, names, font, palette, gw,
                                       int(thickness), int(text_scale), float(margin), bool(show_score), out)
    return out
