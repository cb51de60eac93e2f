"""The scenes of the antialiased-resize tests (``ops/scale.py``), shared by test_scale_reference.py
(``scale_frames_ref`` against Pillow and against a second formulation) and test_gpu_scale.py (the
kernels against ``scale_frames_ref``).  A scene's frames and its reference are computed once per
process and handed out unchanged.

``PAIRS`` lists (H, W, Ho, Wo):

* 480 x 640 -> 224 x 224: the classifier input behind a camera, several tiles in both directions;
* 37 x 53 -> 91 x 17: one axis up and one down, rows of 159 bytes (no 4- or 16-byte alignment);
* 5 x 7 -> 40 x 56: enlargement, the taps clipped at both edges;
* 1 x 1 -> 9 x 9;
* 64 x 64 -> 64 x 31 and -> 31 x 64: one pass only (the kernels without the other pass);
* 97 x 131 -> 70 x 150: a partial last tile in both directions;
* 33 x 65 -> 3 x 5: 79 taps with ``lanczos``;
* 16 x 4100 -> 3 x 7: wide rows, up to 3517 horizontal taps.

Every pair runs with the whole frame and with a box in sixteenths of a pixel that cuts a different
fraction off every side.  The left half of a frame is uniform noise, the right half binary 0 / 255
noise: uniform noise almost never reaches the clamp, and the negative lobes of ``bicubic`` and
``lanczos`` reach it only on hard edges.

A plain module (no fixtures, no device requirement), like kernel_guard.py."""
from __future__ import annotations

import torch

B = 3
FILTER_NAMES = ("box", "bilinear", "hamming", "bicubic", "lanczos")
PAIRS = [(480, 640, 224, 224), (37, 53, 91, 17), (5, 7, 40, 56), (1, 1, 9, 9), (64, 64, 64, 31), (64, 64, 31, 64),
         (97, 131, 70, 150), (33, 65, 3, 5), (16, 4100, 3, 7)]


def box_of(pair):
    """The scene's box (left, top, right, bottom) in sixteenths: 20 / 8 / 12 / 24 sixteenths off the
    four sides where the frame is large enough, a part of the only pixel of the 1 x 1 frame."""
    h, w = pair[:2]
    if h == 1 and w == 1:
        return (2, 3, 14, 16)
    return (20, 8, 16 * w - 12, 16 * h - 24)


CASES = [(pair, f, boxed) for pair in PAIRS for f in FILTER_NAMES for boxed in (False, True)]


def case_id(case):
    (h, w, ho, wo), f, boxed = case
    return f"{h}x{w}-{ho}x{wo}-{f}" + ("-box" if boxed else "")


def box(case):
    return box_of(case[0]) if case[2] else None


_FRAMES = {}


def frames(height, width, seed=0, batch=B):
    """uint8 ``[batch, height, width, 3]``: seeded noise, binary 0 / 255 in the right half."""
    key = (height, width, seed, batch)
    if key not in _FRAMES:
        g = torch.Generator().manual_seed(1000 * seed + 7 * height + width)
        f = torch.randint(0, 256, (batch, height, width, 3), dtype=torch.uint8, generator=g)
        right = f[:, :, width // 2:]
        right.copy_(torch.where(right > 127, 255, 0).to(torch.uint8))
        _FRAMES[key] = f
    return _FRAMES[key]


_REF = {}


def reference(case, seed=0):
    """``scale_frames_ref`` on a case -> uint8 ``[B, Ho, Wo, 3]``, computed once; not to be modified."""
    key = (case_id(case), seed)
    if key not in _REF:
        from aiko_services_amd.ops.reference import scale_frames_ref
        (h, w, ho, wo), f, _ = case
        _REF[key] = scale_frames_ref(frames(h, w, seed), (ho, wo), f, box(case))
    return _REF[key]
