"""Scenes of the marker tests (``ops/marker.py``), shared by test_marker_reference.py (what
``detect_markers_ref`` must find, and what the scenes must cover) and test_gpu_marker.py (the kernels
against ``detect_markers_ref``).  A scene's reference result is computed once per process and handed
out unchanged.

Three frames of 176 x 208 (208: the dword path; 203: the byte path, a partial range block, a partial
cell at every cell size and tail bits in the last word of the packed mask): two tiles across and six
tile rows of the kernels' 128 x 32 tile.  Markers are rendered by inverse projective mapping of the
module grids of ``make_marker_original`` / ``make_marker`` under a 0.55..1.0 left-to-right lighting
ramp; a planted marker is ``(id, quad)``, the quad its outer corners (top-left first, clockwise in
the marker's own frame) in pixel-centre coordinates.

A plain module (no fixtures, no device requirement), like kernel_guard.py."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

B, H, W = 3, 176, 208
W_ODD = 203
WIDTHS = (W, W_ODD)
CELLS = (4, 8)
BLACK, WHITE = 20, 235
BASE = dict(cell=4, contrast=64, min_side=24, max_cand=32, max_det=16)
SLOTS5 = [(x, y) for y in (40, 122) for x in (36, 104, 172)]        # centres of module-5 markers, gaps >= 18 px
SLOTS8 = [(x, y) for y in (43, 133) for x in (52, 150)]             # centres of module-8 markers (not at 45 degrees)


def grid(cell, width=W, height=H):
    return -(-height // cell), -(-width // cell)


def module_grid(dictionary, marker_id):
    """The N x N modules (1 = white) of a marker, border included."""
    from aiko_services_amd.examples.aruco_marker.aruco import make_marker, make_marker_original
    make = make_marker_original if dictionary == "original" else make_marker
    return (make(marker_id, cell=1, quiet=0) > 0).astype(np.uint8)


def canonical16(code):
    """The smallest payload over the four rotations of the 4 x 4 payload ``code``: the id it is found under."""
    bits = np.array([(code >> i) & 1 for i in range(16)], np.uint8).reshape(4, 4)
    return min(int(sum(int(v) << i for i, v in enumerate(np.rot90(bits, -r).reshape(-1)))) for r in range(4))


def square(cx, cy, side, angle=0.0, squeeze=1.0):
    """The quad of a square of ``side`` pixels about ``(cx, cy)``, turned clockwise (on the screen) by
    ``angle`` degrees; ``squeeze`` < 1 shortens its right side about the centre line: a view from
    the left."""
    h = side / 2.0
    pts = [(-h, -h), (h, -h * squeeze), (h, h * squeeze), (-h, h)]
    c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    return [(cx + c * x - s * y, cy + s * x + c * y) for x, y in pts]


def aligned(x0, y0, side, turns=0):
    """The quad of an axis-aligned marker on the pixels ``[x0, x0 + side) x [y0, y0 + side)``,
    turned by ``turns`` quarter turns clockwise."""
    q = [(x0 - 0.5, y0 - 0.5), (x0 + side - 0.5, y0 - 0.5), (x0 + side - 0.5, y0 + side - 0.5),
         (x0 - 0.5, y0 + side - 0.5)]
    return [q[(i + turns) % 4] for i in range(4)]


def _homography(quad):
    """3 x 3 float64 map of the unit square's (0,0), (1,0), (1,1), (0,1) onto ``quad``."""
    src = [(0, 0), (1, 0), (1, 1), (0, 1)]
    rows, rhs = [], []
    for (u, v), (x, y) in zip(src, quad):
        rows += [[u, v, 1, 0, 0, 0, -u * x, -v * x], [0, 0, 0, u, v, 1, -u * y, -v * y]]
        rhs += [x, y]
    h = np.linalg.solve(np.array(rows, np.float64), np.array(rhs, np.float64))
    return np.append(h, 1.0).reshape(3, 3)


def paint(gray, modules, quad):
    """The marker ``modules`` on the quad, into the float ``gray`` [H, W] (levels before lighting):
    every pixel whose centre maps into the unit square takes its module's level."""
    inv = np.linalg.inv(_homography(quad))
    h, w = gray.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = inv[2, 0] * xx + inv[2, 1] * yy + inv[2, 2]
    u = (inv[0, 0] * xx + inv[0, 1] * yy + inv[0, 2]) / d
    v = (inv[1, 0] * xx + inv[1, 1] * yy + inv[1, 2]) / d
    n = modules.shape[0]
    inside = (u >= 0) & (u < 1) & (v >= 0) & (v < 1) & (d > 0)
    j, i = np.clip((u * n).astype(int), 0, n - 1), np.clip((v * n).astype(int), 0, n - 1)
    gray[inside] = np.where(modules[i, j] > 0, WHITE, BLACK)[inside]


def light(gray):
    """uint8 [H, W, 3] of the levels ``gray`` under the ramp: 0.55 at the left, 1.0 at the right."""
    w = gray.shape[1]
    ramp = 0.55 + 0.45 * np.arange(w) / max(w - 1, 1)
    g = np.clip(np.rint(gray * ramp[None, :]), 0, 255).astype(np.uint8)
    return torch.from_numpy(np.repeat(g[:, :, None], 3, axis=2).copy())


class Scene:
    """``frames`` uint8 [B, H, width, 3]; ``planted`` per frame the findable markers [(id, quad)];
    ``kw`` the parameters."""

    def __init__(self, name, width):
        self.name, self.width = name, width
        self.kw = dict(BASE, dictionary="original")
        self.planted = [[] for _ in range(B)]
        self.gray = [np.full((H, width), float(WHITE)) for _ in range(B)]
        self.counts = self.cands = None                     # per frame, where the caps make them differ
        getattr(self, "_" + name)()
        self.frames = torch.stack([light(g) for g in self.gray])
        del self.gray

    def plant(self, b, marker_id, quad, findable=True, modules=None):
        paint(self.gray[b], module_grid(self.kw["dictionary"], marker_id) if modules is None else modules, quad)
        if findable:
            self.planted[b].append((marker_id, quad))

    # every 15 degrees: 0..150 here, 165..315 in angles_b, 330, 345 and 45 again (module 8) in large
    def _angles_a(self):
        for k in range(11):
            b, (cx, cy) = (0, SLOTS5[k]) if k < 6 else (1, SLOTS5[k - 6])
            self.plant(b, 37 + 91 * k, square(cx, cy, 35, 15 * k))

    def _angles_b(self):
        for k in range(11):
            b, (cx, cy) = (1, SLOTS5[k]) if k < 6 else (2, SLOTS5[k - 6])
            self.plant(b, 1000 - 57 * k, square(cx + 0.5, cy + 0.25, 35, 165 + 15 * k))

    def _large(self):
        for k, angle in enumerate((330, 345, 20, 70)):
            self.plant(0, 5 + 200 * k, square(*SLOTS8[k], 56, angle))
        self.plant(2, 682, square(70, 88, 56, 45))                         # exactly 45: the axial quad
        self.plant(2, 341, square(160, 60, 64, 10, squeeze=0.6))           # foreshortened to 0.6 on one side

    def _upright(self):
        for k in range(4):
            cx, cy = SLOTS8[k]
            self.plant(0, 100 + 7 * k, aligned(cx - 28, cy - 28, 56, turns=k))
        self.plant(1, 1000, aligned(90, 60, 35))

    def _quarter16(self):
        self.kw["dictionary"] = "payload16"
        for k in range(4):
            cx, cy = SLOTS8[k]
            self.plant(0, canonical16(0x08C7 + k), aligned(cx - 24, cy - 24, 48, turns=k))
        self.plant(2, canonical16(0x0137), aligned(20, 30, 30))
        self.plant(2, canonical16(0x0001), square(140, 90, 48, 30))

    def _caps(self):
        self.kw.update(max_cand=4, max_det=2)
        for k in range(6):                                                  # 6 candidates, 4 examined, 2 rows
            self.plant(0, 11 * k, square(*SLOTS5[k], 35, 10 * k), findable=False)
        solid = np.zeros((7, 7), np.uint8)
        for k in range(3):                                                  # three solid squares take three of
            self.plant(1, 0, aligned(20 + 60 * k, 20, 30), findable=False, modules=solid)   # the four examined
        self.plant(1, 77, aligned(30, 100, 35))
        self.plant(1, 78, aligned(120, 100, 35), findable=False)            # the fifth candidate: not examined
        self.counts, self.cands = [2, 1, 0], [6, 5, 0]

    def _edges(self):
        self.plant(0, 300, aligned(1, 1, 35))                               # 1 px inside the frame's corner
        self.plant(0, 301, aligned(self.width - 36, H - 36, 35, turns=2))
        self.plant(0, 302, square(100, 80, 40, 33))
        self.plant(1, 303, aligned(self.width - 28, 60, 35), findable=False)     # cut by the right edge
        self.plant(1, 304, aligned(60, H - 22, 40), findable=False)         # cut by the bottom edge
        broken = module_grid("original", 305)
        broken[0, 3] = 1                                                    # a white module in the border
        self.plant(2, 305, square(60, 60, 40, 20), findable=False, modules=broken)
        bad = module_grid("original", 306)
        bad[1:6, 1:6] = np.array([[1, 1, 0, 0, 1]] * 5)                      # 11001 in every direction: no codeword
        bad[3, 3] = 0
        self.plant(2, 306, square(150, 100, 40, 50), findable=False, modules=bad)

    def _pairs(self):
        self.plant(0, 400, aligned(40, 30, 35))                             # dark pixels up to x = 74
        self.plant(0, 401, aligned(83, 30, 35))                             # 8 white pixels between
        self.plant(1, 402, aligned(40, 30, 35), findable=False)
        self.plant(1, 403, aligned(79, 30, 35), findable=False)             # 4 white pixels: cells 18 and 19 touch
        self.plant(2, 404, square(100, 90, 42, 60))

    def _worst(self):
        g = self.gray[0]                                                    # a serpentine of 8-pixel bands
        for k, y in enumerate(range(0, H, 16)):
            g[y:y + 8, :] = BLACK
            if y + 16 < H:
                g[y + 8:y + 16, self.width - 8:] = BLACK if k % 2 == 0 else WHITE
                g[y + 8:y + 16, :8] = BLACK if k % 2 == 1 else WHITE
        self.gray[1][20:110, 15:105] = BLACK                                # 90 x 90: holes in its dark mask
        self.plant(1, 500, square(160, 120, 35, 25))
        rng = np.random.default_rng(7)
        self.gray[2][:] = rng.integers(0, 256, (H, self.width))             # uniform noise

    def _negatives(self):
        rng = np.random.default_rng(11)                                     # frame 0 stays blank
        blocks = rng.integers(0, 2, (H // 8, -(-self.width // 8)))
        self.gray[1][:] = np.kron(blocks, np.ones((8, 8)))[:, :self.width] * (WHITE - BLACK) + BLACK
        self.gray[2][:] = 128                                               # grey with faint texture: no contrast
        self.gray[2][::2, ::3] = 150


NAMES = ("angles_a", "angles_b", "large", "upright", "quarter16", "caps", "edges", "pairs", "worst", "negatives")
ALIGNED = ("upright", "quarter16")                          # what detect_markers_numpy finds too


@functools.lru_cache(maxsize=None)
def scene(name, width=W):
    return Scene(name, width)


@functools.lru_cache(maxsize=None)
def reference(name, width=W, cell=4):
    """``(det, count, corners, ids, cands, mask)`` of ``detect_markers_ref``; computed once, not to
    be modified."""
    from aiko_services_amd.ops.reference import detect_markers_ref
    s = scene(name, width)
    return detect_markers_ref(s.frames, **{**s.kw, "cell": cell})
