"""Antialiased resize (``csrc/kernels/scale_ops.hip``): uint8 ``[B, H, W, 3]`` frames to any size,
smaller or larger, with a separable pre-filter in fixed point.  Every byte equals Pillow's
``Image.resize`` with the same filter, which is what the host path of ``ImageResize`` and
torchvision-style preprocessing use, so a pipeline gives the same picture on either side of the
device boundary.  ``ops.vision.resize_u8`` stays what it is: two taps per axis, no pre-filter.

The rule (kernel and ``ops.reference.scale_frames_ref`` both follow it; once the coefficient tables
exist everything is integer, so they agree bit for bit):

* **Filters.**  Each has a ``support`` and an ``f(x)``, evaluated in float64 in exactly this order of
  operations with ``math.sin``, ``math.cos`` and ``math.pi`` (the C library's, which Pillow calls):

  ============  =======  ==========================================================================
  ``box``       0.5      1 if ``-0.5 < x <= 0.5``, else 0
  ``bilinear``  1        ``x = abs(x)``; ``1.0 - x`` if ``x < 1``, else 0
  ``hamming``   1        ``x = abs(x)``; 1 if ``x == 0``; 0 if ``x >= 1``; else ``x = x*pi;
                         sin(x)/x * (A + B*cos(x))``
  ``bicubic``   2        ``a = -0.5; x = abs(x)``; ``((a+2.0)*x - (a+3.0))*x*x + 1`` if ``x < 1``;
                         ``(((x-5)*x + 8)*x - 4)*a`` if ``x < 2``; else 0
  ``lanczos``   3        ``sinc(x)*sinc(x/3)`` if ``-3 <= x < 3``, else 0; ``sinc(0) = 1``,
                         otherwise ``x = x*pi; sin(x)/x``
  ============  =======  ==========================================================================

  A and B of ``hamming`` are the float32 values of 0.54 and 0.46 widened to double (Pillow's source
  writes ``0.54f``); with the double constants about one image in sixty differs by one level.
* **Axis plan.**  From ``in_size``, ``out_size``, a filter and the box edges ``a0 < a1`` in
  sixteenths of a pixel, ``0 <= a0 < a1 <= 16*in_size`` (default: the whole axis).  Sixteenths,
  because Pillow holds the box in float32 and subtracts there: sixteenths of sizes up to ``2**20``
  are exact in float32 and float64 alike, arbitrary float boxes do not reproduce. ::

      in0 = a0/16.0 ; in1 = a1/16.0
      scale = (in1 - in0) / out_size ; fs = max(scale, 1.0) ; sup = support * fs
      ksize = ceil(sup)*2 + 1 ; inv = 1.0 / fs
      for xx in 0..out_size-1:
          center = in0 + (xx + 0.5) * scale
          first  = max(int(center - sup + 0.5), 0)        # int() truncates towards zero
          n      = min(int(center + sup + 0.5), in_size) - first
          w[x]   = f((x + first - center + 0.5) * inv)    for x in 0..n-1
          ww     = w[0] + w[1] + ...  (in this order) ;  if ww != 0: w[x] = w[x] / ww
          k[x]   = int(w[x]*4194304 + 0.5) if w[x] >= 0 else int(w[x]*4194304 - 0.5)   # 22 bits

  No fused multiply-add appears anywhere in the plan (Python has none).
* **A pass.**  Per channel ``out = clamp((2**21 + sum_x k[x] * p[first + x]) >> 22, 0, 255)`` with an
  arithmetic shift (a floor).  The sum fits int32 when ``255 * sum|k| + 2**21 < 2**31``; the plan
  maker checks that per output position and raises otherwise.  The five filters never reach it.
* **Order.**  The horizontal pass runs over the source rows and gives a uint8 intermediate
  ``[H, Wo, 3]``, rounded and clamped as Pillow's is, which is why the two passes cannot be one sum;
  the vertical pass runs on the intermediate.  A pass whose axis has ``out_size == in_size`` and the
  whole-axis box is left out: its coefficients would be the identity.
* **Limits.**  Sizes from 1 to ``MAX_SIDE`` = ``2**20``; ``ksize <= MAX_TAPS`` = 4097 per axis, which is
  ``lanczos`` at 682:1 and ``box`` at 4096:1.  At ``MAX_TAPS`` rows the source window of one output
  row, twelve columns wide, still fits the 160 KiB of LDS of a CU.  Anything beyond is a
  ``ValueError`` that names the limit; enlargement has no limit other than the sizes.

On the device a workgroup makes a tile of ``tile_rows`` x ``tile_cols`` output pixels: the horizontal
pass of the tile's source rows into LDS, then the vertical pass out of LDS.  :func:`scale_plan`
chooses the tile so that the window fits 32 KiB where it can (several workgroups per CU) and the
whole 160 KiB where it must, builds both tables and uploads them once per set of arguments.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np
import torch

__all__ = ["FILTERS", "MAX_SIDE", "MAX_TAPS", "ScalePlan", "axis_plan", "box_from_pixels", "check_size",
           "scale_frames", "scale_plan", "tile_for"]

PRECISION_BITS = 22
MAX_TAPS = 4097
MAX_SIDE = 1 << 20
MAX_FRAMES = 65535           # a grid's third dimension
MAX_LDS = 160 * 1024
TILE_LDS = 32 * 1024         # what a tile's window should fit: four workgroups or more per CU
TILE_ROWS = 64               # output rows of a tile, at most
TILE_COLS = (64, 32, 16, 12, 8, 4)

_HAMMING_A = float(np.float32(0.54))
_HAMMING_B = float(np.float32(0.46))


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_HAMMING_A + _HAMMING_B * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# name -> (support, f)
FILTERS = {"box": (0.5, _box), "bilinear": (1.0, _bilinear), "hamming": (1.0, _hamming),
           "bicubic": (2.0, _bicubic), "lanczos": (3.0, _lanczos)}


def _integer(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"scale_frames: {name} must be an integer, got {v!r}")
    return int(v)


def axis_plan(in_size: int, out_size: int, filter: str = "bicubic", a0: int | None = None, a1: int | None = None):
    """``(bounds, k)`` of one axis by the rule in this module's docstring: int32 ``[out_size, 2]``
    (``first``, ``n``) and int32 ``[out_size, ksize]`` (a row's coefficients past ``n`` are 0).
    ``a0`` / ``a1``: the box edges in sixteenths of a pixel, by default the whole axis.  Raises
    ``ValueError`` for an unknown filter, sizes outside 1..``MAX_SIDE``, a box outside the axis,
    ``ksize > MAX_TAPS`` and coefficients whose sums would leave int32."""
    if filter not in FILTERS:
        raise ValueError(f"scale_frames: filter one of {sorted(FILTERS)} required, got {filter!r}")
    in_size, out_size = _integer("in_size", in_size), _integer("out_size", out_size)
    if not 1 <= in_size <= MAX_SIDE or not 1 <= out_size <= MAX_SIDE:
        raise ValueError(f"scale_frames: sizes from 1 to {MAX_SIDE} required, got {in_size} -> {out_size}")
    a0 = 0 if a0 is None else _integer("box", a0)
    a1 = 16 * in_size if a1 is None else _integer("box", a1)
    if not 0 <= a0 < a1 <= 16 * in_size:
        raise ValueError(f"scale_frames: box edges 0 <= a0 < a1 <= {16 * in_size} (sixteenths of the {in_size} "
                         f"pixels) required, got {a0}, {a1}")
    support, f = FILTERS[filter]
    in0, in1 = a0 / 16.0, a1 / 16.0
    scale = (in1 - in0) / out_size
    fs = max(scale, 1.0)
    sup = support * fs
    ksize = math.ceil(sup) * 2 + 1
    if ksize > MAX_TAPS:
        raise ValueError(f"scale_frames: {filter} at {scale:.1f}:1 needs {ksize} taps, more than MAX_TAPS = "
                         f"{MAX_TAPS}")
    inv = 1.0 / fs
    one = float(1 << PRECISION_BITS)
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        first = max(int(center - sup + 0.5), 0)
        n = min(int(center + sup + 0.5), in_size) - first
        if not (0 <= n <= ksize and first + n <= in_size):          # the rule implies it
            raise ValueError(f"scale_frames: position {xx} reads [{first}, {first + n}) of {in_size}")
        w = [f((x + first - center + 0.5) * inv) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        row = [int(v * one + 0.5) if v >= 0 else int(v * one - 0.5) for v in w]
        if 255 * sum(abs(v) for v in row) + (1 << (PRECISION_BITS - 1)) >= 1 << 31:
            raise ValueError(f"scale_frames: the coefficients of position {xx} sum to more than int32 holds")
        bounds[xx] = (first, n)
        k[xx, :n] = row
    return bounds, k


def check_size(size):
    """``size`` = (Ho, Wo) as two integers of 1..``MAX_SIDE``, or ``ValueError``."""
    try:
        size = tuple(size)
    except TypeError:
        size = ()
    if len(size) != 2:
        raise ValueError(f"scale_frames: size = (height, width) required, got {size!r}")
    Ho, Wo = _integer("size", size[0]), _integer("size", size[1])
    if not 1 <= Ho <= MAX_SIDE or not 1 <= Wo <= MAX_SIDE:
        raise ValueError(f"scale_frames: sizes from 1 to {MAX_SIDE} required, got {Ho} x {Wo}")
    return Ho, Wo


def check_box(H: int, W: int, box):
    """``box`` = (left, top, right, bottom) in sixteenths of a pixel inside an H x W frame, as four
    integers, or ``None`` for the whole frame (also when the box is the whole frame)."""
    if box is None:
        return None
    try:
        box = tuple(box)
    except TypeError:
        box = ()
    if len(box) != 4:
        raise ValueError(f"scale_frames: box = (left, top, right, bottom) in sixteenths required, got {box!r}")
    left, top, right, bottom = (_integer("box", v) for v in box)
    if not (0 <= left < right <= 16 * W and 0 <= top < bottom <= 16 * H):
        raise ValueError(f"scale_frames: box {box} lies outside the frame, (0, 0, {16 * W}, {16 * H}) in sixteenths, "
                         "or is empty")
    return None if (left, top, right, bottom) == (0, 0, 16 * W, 16 * H) else (left, top, right, bottom)


def box_from_pixels(box):
    """(left, top, right, bottom) in pixels, multiples of 1/16, as the integers in sixteenths that
    :func:`scale_frames` takes; ``ValueError`` for anything else."""
    try:
        values = [float(v) for v in box]
    except (TypeError, ValueError):
        values = []
    if len(values) != 4 or any(isinstance(v, bool) for v in box) or not all(math.isfinite(v) for v in values):
        raise ValueError(f"scale_frames: box = four numbers (left, top, right, bottom) in pixels required, got {box!r}")
    if any(v * 16.0 != math.floor(v * 16.0) or abs(v) > MAX_SIDE for v in values):
        raise ValueError(f"scale_frames: box edges must be multiples of 1/16 pixel, got {box!r}")
    return tuple(int(v * 16.0) for v in values)


def axis_plans(H: int, W: int, size, filter: str = "bicubic", box=None):
    """``(horizontal, vertical)``: each :func:`axis_plan`'s tables, or ``None`` where the rule leaves
    the pass out (same size, whole-axis box)."""
    Ho, Wo = check_size(size)
    H, W = _integer("H", H), _integer("W", W)
    if not 1 <= H <= MAX_SIDE or not 1 <= W <= MAX_SIDE:
        raise ValueError(f"scale_frames: sizes from 1 to {MAX_SIDE} required, got frames of {H} x {W}")
    if filter not in FILTERS:
        raise ValueError(f"scale_frames: filter one of {sorted(FILTERS)} required, got {filter!r}")
    box = check_box(H, W, box) or (0, 0, 16 * W, 16 * H)
    horizontal = vertical = None
    if Wo != W or (box[0], box[2]) != (0, 16 * W):
        horizontal = axis_plan(W, Wo, filter, box[0], box[2])
    if Ho != H or (box[1], box[3]) != (0, 16 * H):
        vertical = axis_plan(H, Ho, filter, box[1], box[3])
    return horizontal, vertical


def window_rows(bounds: np.ndarray, tile_rows: int) -> int:
    """The most source rows that ``tile_rows`` consecutive output rows (tiles start at multiples of
    ``tile_rows``) read between the first one's ``first`` and the last one's ``first + n``."""
    n_out = bounds.shape[0]
    start = np.arange(0, n_out, tile_rows)
    last = np.minimum(start + tile_rows, n_out) - 1
    return int((bounds[last, 0] + bounds[last, 1] - bounds[start, 0]).max())


def tile_for(bounds: np.ndarray):
    """``(tile_rows, tile_cols, win_rows)`` for a vertical plan's bounds: the widest tile of
    ``TILE_COLS``, and with it the tallest up to ``TILE_ROWS`` rows, whose window of ``win_rows``
    source rows x ``tile_cols`` columns x 3 bytes fits ``TILE_LDS``; failing that, ``MAX_LDS``."""
    for budget in (TILE_LDS, MAX_LDS):
        for cols in TILE_COLS:
            for rows in range(min(TILE_ROWS, bounds.shape[0]), 0, -1):
                win = window_rows(bounds, rows)
                if win * cols * 3 <= budget:
                    return rows, cols, max(win, 1)
    raise ValueError(f"scale_frames: a window of {window_rows(bounds, 1)} rows does not fit {MAX_LDS} bytes of LDS")


class ScalePlan(NamedTuple):
    """What :func:`scale_frames` hands the operator for one (H, W, size, filter, box, device): the
    tables on the device (``None`` for a pass that is left out), the tile and the most source rows a
    tile reads."""
    size: tuple
    hb: torch.Tensor | None
    hk: torch.Tensor | None
    vb: torch.Tensor | None
    vk: torch.Tensor | None
    tile_rows: int
    tile_cols: int
    win_rows: int


@functools.lru_cache(maxsize=None)           # never evicted: a captured graph may point at a plan's tables
def _scale_plan(H, W, size, filter, box, device):
    horizontal, vertical = axis_plans(H, W, size, filter, box)
    up = lambda t: None if t is None else torch.from_numpy(t).to(device)  # noqa: E731
    tile = tile_for(vertical[0]) if horizontal is not None and vertical is not None else (1, 4, 1)
    return ScalePlan(size, *(up(t) for t in (horizontal or (None, None))), *(up(t) for t in (vertical or (None, None))),
                     *tile)


def scale_plan(H: int, W: int, size, filter: str = "bicubic", box=None, device="cuda") -> ScalePlan:
    """Both axes' tables for H x W frames scaled to ``size`` = (Ho, Wo), built by :func:`axis_plan`
    and uploaded to ``device`` once.  Cached: the same arguments return the same tensors, which
    callers must not modify, so nothing is uploaded inside a captured region after the first call.
    The cache has no size limit and a plan is never evicted, because a captured graph keeps reading
    the tables it was captured with: a process holds one pair of tables (a few KB to a few MB) for
    every (shape, size, filter, box, device) it has ever scaled."""
    size = check_size(size)
    box = check_box(int(H), int(W), box)
    return _scale_plan(int(H), int(W), size, filter, box, str(torch.device(device)))


def scale_frames(frames: torch.Tensor, size, filter: str = "bicubic", box=None,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 ``[B, H, W, 3]`` frames on the device -> uint8 ``[B, Ho, Wo, 3]``: the part of every frame
    inside ``box`` = (left, top, right, bottom), in sixteenths of a pixel (default: all of it), scaled
    to ``size`` = (Ho, Wo) with ``filter`` by the rule in this module's docstring.  ``out`` is written
    if given and may not overlap ``frames``.  The same size with no box is a copy."""
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("scale_frames: frames uint8 [B, H, W, 3] required")
    B, H, W = (int(v) for v in frames.shape[:3])
    if not 1 <= B <= MAX_FRAMES:
        raise ValueError(f"scale_frames: 1 to {MAX_FRAMES} frames required, got {B}")
    plan = scale_plan(H, W, size, filter, box, frames.device)
    if out is None:
        out = torch.empty(B, *plan.size, 3, dtype=torch.uint8, device=frames.device)
    if plan.hb is None and plan.vb is None:
        if tuple(out.shape) != tuple(frames.shape) or out.dtype != frames.dtype:
            raise ValueError(f"scale_frames: out uint8 {tuple(frames.shape)} required, got {tuple(out.shape)}")
        out.copy_(frames)
        return out
    torch.ops.aiko.scale_frames_out(frames, plan.hb, plan.hk, plan.vb, plan.vk, plan.tile_rows, plan.tile_cols,
                                    plan.win_rows, out)
    return out
