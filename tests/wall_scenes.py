"""The scenes of the camera-wall tests (``ops/wall.py``), shared by test_wall_reference.py (what
``frame_wall_ref`` must give) and test_gpu_wall.py (the kernels against ``frame_wall_ref``).  All
frames are seeded noise; a configuration's reference is computed once per process and handed out
unchanged.

The base scene: seven cameras of 50 x 131 (a row is 393 bytes: the byte path) and the same at
50 x 128 (the 16-byte path), scores [3, 0, 5, 5, -2, 1, 0], a grid of 2 x 3 on two pages, so that
index order leaves five slots empty and score order eight.  ``CASES`` lists (H, W, tile):

* (13, 37): non-integer ratios, source rows and columns shared by two output pixels;
* the identity tile (a copy), (1, 1) (the mean of the frame), (50, 1) and (1, W);
* 48 x 128 at (12, 32): the integer factor 4, the redaction's cell colour;
* 9 x 301 at (9, 300): a tile row wider than a workgroup;
* 3 x 5008 at (2, 2) and 3 x 5000 at (1, 2): one output column spans more source columns than an
  LDS segment of the kernel holds (2048), so its sum is carried over segments, on both paths.

A plain module (no fixtures, no device requirement), like kernel_guard.py."""
from __future__ import annotations

import torch

B, H, W = 7, 50, 131
W16 = 128
SCORES = [3, 0, 5, 5, -2, 1, 0]
ROWS, COLS, PAGES = 2, 3, 2
N = ROWS * COLS
SCORE_ORDER = [2, 3, 0, 5]                      # score >= 1, descending, ties to the lower index
COLOURS = dict(background=(10, 20, 30), alert=(250, 40, 5), label_fg=(255, 255, 0), label_bg=(0, 0, 64))

CASES = [(H, w, t) for w in (W, W16) for t in ((13, 37), (H, w), (1, 1), (H, 1), (1, w))] + \
    [(48, 128, (12, 32)), (9, 301, (9, 300)), (3, 5008, (2, 2)), (3, 5000, (1, 2))]

# gap, ring (cut to what the tile allows), label_scale, label_base: plain; everything on (numbers
# 0..6); scale 3 with the two-digit numbers 93..99, so that between them every digit is drawn
OPTIONS = [dict(gap=0, ring=0, label_scale=0, label_base=0),
           dict(gap=3, ring=2, label_scale=1, label_base=0),
           dict(gap=1, ring=1, label_scale=3, label_base=93)]


def case_id(case):
    h, w, (th, tw) = case
    return f"{h}x{w}-{th}x{tw}"


def options(case, i):
    """``OPTIONS[i]`` with the ring cut to ``min(tile) // 2``."""
    o = dict(OPTIONS[i])
    o["ring"] = min(o["ring"], min(case[2]) // 2)
    return o


_FRAMES = {}


def frames(height=H, width=W, seed=0):
    """uint8 ``[B, height, width, 3]`` noise from ``seed`` (made once per shape and seed)."""
    key = (height, width, seed)
    if key not in _FRAMES:
        g = torch.Generator().manual_seed(1000 * seed + height + width)
        _FRAMES[key] = torch.randint(0, 256, (B, height, width, 3), dtype=torch.uint8, generator=g)
    return _FRAMES[key]


def scores(values=SCORES):
    return torch.tensor(values, dtype=torch.int32)


_REF = {}


def reference(case, order="index", opt=0, with_score=True):
    """``frame_wall_ref`` on a case of the shared scene -> (wall, source), computed once per
    configuration; not to be modified."""
    key = (case_id(case), order, opt, with_score)
    if key not in _REF:
        from aiko_services_amd.ops.reference import frame_wall_ref
        h, w, tile = case
        _REF[key] = frame_wall_ref(frames(h, w), scores() if with_score else None, rows=ROWS, cols=COLS, tile=tile,
                                   pages=PAGES, order=order, **options(case, opt), **COLOURS)
    return _REF[key]
