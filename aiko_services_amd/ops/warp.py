"""Projective warp of uint8 frames, selected by quads on the device (``csrc/kernels/warp_ops.hip``):
``K`` quads per frame and their count are read where they lie in HBM (the ``marker_corners`` /
``counts`` of ``MarkerDetector``, as ``roi_crop`` reads the detector's rows) and ``K`` rectified
patches per frame are written.  One launch, no host copy, no synchronisation, hipGraph-capturable.
With one fixed quad per camera the same kernel turns, flips, keystone-corrects or pans whole frames
(:func:`view_quad`).

The rule.  :func:`~aiko_services_amd.ops.reference.warp_quads_ref` is the same in numpy float64 and
equals the kernel bit for bit.

**Inputs.**  ``frames`` uint8 ``[B, H, W, 3]``, contiguous, ``H, W <= 4096``.  ``quads`` int32 ``[B, Kq,
4, 2]`` as ``(x, y)``, in the order ``C0..C3`` = the patch's top-left, top-right, bottom-right,
bottom-left (the order of ``marker_corners``).  ``count`` int32 ``[B]``, read on the device.  ``1 <= k
<= Kq``.  ``size`` = ``(Ho, Wo)``, ``Wo % 4 == 0``, ``1 <= Ho, Wo <= 4096``.  ``margin``: an integer
``m`` in ``0..64``, sixteenths of the quad's side added on every side.  ``origin``: ``"centre"`` (the
coordinates are pixel indices, a corner is a pixel's centre: what ``MarkerDetector`` emits) or
``"edge"`` (the coordinates are pixel edges: the frame is the quad ``(0,0) (W,0) (W,H) (0,H)``).

**Outputs.**  ``patches`` uint8 ``[B*k, Ho, Wo, 3]`` and ``valid`` int32 ``[B*k]``; slot ``b*k + i`` is
quad ``i`` of frame ``b``.  Every element of both is written on every call.

1. **Used slots.**  Slot ``(b, i)`` is used iff ``i < min(max(count[b], 0), k)``, all eight
   coordinates lie in ``-4096..8191`` and ``den != 0`` (below).  An unused slot is all zeros and its
   ``valid`` is 0; a used slot's ``valid`` is 1.
2. **Coefficients, exact in int64.**  ``o`` = 1 for ``centre``, 0 for ``edge``; ``Xn = 2*xn + o``, ``Yn =
   2*yn + o``: doubled continuous coordinates.  As in ``ops/marker.py`` rule 7: ``dx1 = X1-X2``, ``dx2 =
   X3-X2``, ``sx = X0-X1+X2-X3`` (likewise in ``y``), ``den = dx1*dy2 - dy1*dx2``, ``G = sx*dy2 -
   sy*dx2``, ``Hh = dx1*sy - dy1*sx``, ``A = den*(X1-X0) + G*X1``, ``Bx = den*(X3-X0) + Hh*X3``, ``Cx =
   den*X0``, ``D = den*(Y1-Y0) + G*Y1``, ``E = den*(Y3-Y0) + Hh*Y3``, ``Cy = den*Y0``.  If ``den < 0``
   all nine are negated.  With the coordinate range of step 1 every one of them is below 2^53 in
   magnitude, so its conversion to double is exact.
3. **Per patch pixel** ``(i, j)``.  Integers: ``ua = (2j+1)*(8+m) - m*Wo``, ``ud = 16*Wo``, ``va =
   (2i+1)*(8+m) - m*Ho``, ``vd = 16*Ho``.  Then in fp64, every operation rounded once, in this order,
   with no contraction: ``u = ua / ud``, ``v = va / vd``, ``w = ((G*u) + (Hh*v)) + den``, ``X = ((A*u) +
   (Bx*v)) + Cx``, ``Y = ((D*u) + (E*v)) + Cy``.  If not ``w > 0`` the pixel is ``(0, 0, 0)``.
   Otherwise ``px = X / w``, ``py = Y / w``, ``tx = min(max(px*128 - 127.5, 0), (W-1)*256)``, ``ty``
   likewise with ``H``, ``Px = (int) floor(tx)``, ``Py = (int) floor(ty)``: the position in 1/256 of
   a pixel, rounded to nearest.
4. **Sampling, all integer.**  ``xi = Px >> 8``, ``fx = Px & 255``, ``xj = min(xi+1, W-1)``, likewise
   in ``y``.  Per channel: ``((256-fx)*(256-fy)*p[yi][xi] + fx*(256-fy)*p[yi][xj] + (256-fx)*fy*p[yj][xi]
   + fx*fy*p[yj][xj] + 32768) >> 16``.

Positions outside the frame are clamped to its edge (step 3), so a margin never reads out of bounds.
"""
from __future__ import annotations

import torch

__all__ = ["COORD_MAX", "COORD_MIN", "MAX_MARGIN", "MAX_SIDE", "ORIGINS", "VIEWS", "check_parameters", "view_quad",
           "warp_quads"]

MAX_SIDE = 4096                                         # H, W, Ho, Wo
COORD_MIN, COORD_MAX = -4096, 8191                      # a used quad's coordinates: step 2 stays below 2^53
MAX_MARGIN = 64                                         # sixteenths of the side
ORIGINS = {"centre": 1, "edge": 0}                      # the rule's ``o``
VIEWS = ("identity", "flip_h", "flip_v", "rot90", "rot180", "rot270")


def _is_int(v) -> bool:
    return hasattr(v, "__index__") and not isinstance(v, bool)          # Python and numpy integers


def check_parameters(k, size, margin, origin) -> None:
    """The value ranges of the rule's parameters, as ``ValueError``."""
    if not _is_int(k) or int(k) < 1:
        raise ValueError(f"warp_quads: k an integer >= 1 required, got {k!r}")
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(_is_int(s) for s in size):
        raise ValueError(f"warp_quads: size (Ho, Wo) of two integers required, got {size!r}")
    Ho, Wo = int(size[0]), int(size[1])
    if not (1 <= Ho <= MAX_SIDE and 1 <= Wo <= MAX_SIDE):
        raise ValueError(f"warp_quads: 1 <= Ho, Wo <= {MAX_SIDE} required, got {Ho} x {Wo}")
    if Wo % 4:
        raise ValueError(f"warp_quads: the patch width must be a multiple of 4, got {Wo}")
    if not _is_int(margin) or not 0 <= int(margin) <= MAX_MARGIN:
        raise ValueError(f"warp_quads: margin an integer in 0..{MAX_MARGIN} (sixteenths of the side) required, "
                         f"got {margin!r}")
    if origin not in ORIGINS:
        raise ValueError(f"warp_quads: origin one of {tuple(ORIGINS)} required, got {origin!r}")


def view_quad(name: str, H: int, W: int):
    """``(quad, (Ho, Wo))`` of a named view of an ``H`` x ``W`` frame: the quad ``[(x, y)] * 4`` in edge
    coordinates that the patch's top-left, top-right, bottom-right and bottom-left corners come from,
    and the natural output size.  ``rot90`` turns the picture clockwise by a quarter (``np.rot90(x,
    -1)``), ``rot270`` counter-clockwise; both swap the sides.  At the natural size every view is an
    exact permutation of the pixels."""
    if name not in VIEWS:
        raise ValueError(f"view_quad: view one of {VIEWS} required, got {name!r}")
    if not _is_int(H) or not _is_int(W) or not (1 <= int(H) <= MAX_SIDE and 1 <= int(W) <= MAX_SIDE):
        raise ValueError(f"view_quad: 1 <= H, W <= {MAX_SIDE} required, got {H!r}, {W!r}")
    H, W = int(H), int(W)
    tl, tr, br, bl = (0, 0), (W, 0), (W, H), (0, H)
    quad = {"identity": [tl, tr, br, bl], "flip_h": [tr, tl, bl, br], "flip_v": [bl, br, tr, tl],
            "rot180": [br, bl, tl, tr], "rot90": [bl, tl, tr, br], "rot270": [tr, br, bl, tl]}[name]
    return quad, ((W, H) if name in ("rot90", "rot270") else (H, W))


def warp_quads(frames: torch.Tensor, quads: torch.Tensor, count: torch.Tensor, k: int = 4,
               size: tuple[int, int] = (224, 224), margin: int = 0, origin: str = "centre",
               patches: torch.Tensor | None = None, valid: torch.Tensor | None = None):
    """uint8 ``[B, H, W, 3]`` ``frames`` + ``quads`` int32 ``[B, Kq, 4, 2]`` / ``count`` int32 ``[B]`` ->
    ``(patches, valid)``: uint8 ``[B*k, Ho, Wo, 3]`` and int32 ``[B*k]`` (the rule: this module's
    docstring).  Parameters out of range are a ``ValueError``; shapes, dtypes, devices, overlap and
    alignment are refused by the operator.  ``count`` is read on the device: no host
    synchronisation."""
    check_parameters(k, size, margin, origin)
    if frames.dim() != 4:
        raise ValueError(f"warp_quads: frames [B, H, W, 3] required, got {tuple(frames.shape)}")
    B = frames.shape[0]
    Ho, Wo = int(size[0]), int(size[1])
    if patches is None:
        patches = torch.empty(B * int(k), Ho, Wo, 3, dtype=torch.uint8, device=frames.device)
    elif patches.dim() != 4 or tuple(patches.shape[1:3]) != (Ho, Wo):
        raise ValueError(f"warp_quads: patches [B*k, {Ho}, {Wo}, 3] required, got {tuple(patches.shape)}")
    if valid is None:
        valid = torch.empty(B * int(k), dtype=torch.int32, device=frames.device)
    torch.ops.aiko.quad_warp_out(frames, quads, count, int(k), int(margin), ORIGINS[origin], patches, valid)
    return patches, valid
