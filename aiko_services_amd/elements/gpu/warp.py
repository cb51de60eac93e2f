"""Projective warps on the device: upright patches of the quads a detector found, and turned, flipped
or keystone-corrected views of whole frames, with no host round trip.

    "(SyntheticFrames MarkerDetector (QuadRectify JpegEncode (crops: images)) JpegResults)"
    "(SyntheticFrames FrameWarp YoloDetector DetectionOverlay)"        FrameWarp view: rot180

* ``QuadRectify`` — ``images`` uint8 ``[B, H, W, 3]`` + the ``MarkerDetector``'s ``marker_corners`` int32
  ``[B, max_det, 4, 2]`` / ``counts`` int32 ``[B]`` -> ``crops`` uint8 ``[B*quads, S, S, 3]`` (the first
  ``quads`` quads of every frame, each rectified to ``image_size`` with its own top-left corner at the
  patch's top-left; zeros where a frame has fewer or a quad is degenerate) and ``crops_valid`` int32
  ``[B*quads]`` (1 for a rectified slot); ``counts`` and ``images`` pass through.  The
  ``(crops: images)`` mapping on the edge behind it feeds a classifier or ``JpegEncode`` the patches, as
  behind ``RoiCrop``.  One launch of ``warp_ops.hip``
  (:func:`~aiko_services_amd.ops.warp.warp_quads`, which states the rule) reads the quads and the counts
  on the device: nothing is copied to the host and nothing synchronises, so the element replays inside
  hipGraphs and frame lanes.  One buffer pair per (shape, lane).
* ``FrameWarp`` — ``images`` uint8 ``[B, H, W, 3]`` -> ``images`` uint8 ``[B, Ho, Wo, 3]``: one fixed quad per
  camera (batch row ``b`` is camera ``b``) applied to whole frames: flips and quarter turns (exact pixel
  permutations), keystone correction, digital pan and zoom.

Parameters of ``QuadRectify`` (scalars): ``quads`` (4 patches per frame), ``image_size`` (224, a multiple
of 4), ``margin`` (0; 0..64 sixteenths of the quad's side added on every side).

Parameters of ``FrameWarp``: ``view`` (``identity``; a name of :func:`~aiko_services_amd.ops.warp.view_quad`
— ``identity``, ``flip_h``, ``flip_v``, ``rot90`` (clockwise), ``rot180``, ``rot270`` — or eight integers
``[x0, y0, x1, y1, x2, y2, x3, y3]`` in edge coordinates, the frame being ``(0,0) (W,0) (W,H) (0,H)``: where
the output's top-left, top-right, bottom-right and bottom-left corners lie in the frame; or one such
list per camera), ``size`` (``[Ho, Wo]``; by default the view's natural size: the frame's own, its sides
swapped by a quarter turn).  ``Wo`` must be a multiple of 4.  Element parameters are scalars, so in a
pipeline definition the lists are JSON text: ``"view": "[64, 0, 576, 0, 640, 480, 0, 480]"``, ``"size":
"[480, 640]"``.
"""
from __future__ import annotations

import json

import torch

from ...gpu.element import GpuPipelineElement
from ...pipeline.stream import StreamEvent

__all__ = ["FrameWarp", "QuadRectify"]


def _frames_diagnostic(who, images, max_side):
    """None for uint8 ``[B, H, W, 3]`` contiguous frames on the device within ``max_side``, else the
    diagnostic."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[-1] != 3 or \
            images.dtype != torch.uint8 or images.device.type != "cuda" or not images.is_contiguous():
        return (f"{who}: images uint8 [B, H, W, 3] contiguous on the device required, got "
                f"{tuple(getattr(images, 'shape', ()))} {getattr(images, 'dtype', type(images).__name__)}")
    B, H, W = images.shape[:3]
    if H > max_side or W > max_side or B * H * W * 3 < 4:
        return f"{who}: {H} x {W} frames are past the limits (at most {max_side} pixels a side, at least 4 bytes)"
    return None


class QuadRectify(GpuPipelineElement):
    lane_safe = True          # output buffers per lane

    def __init__(self, context):
        context.set_protocol("quad_rectify:0")
        super().__init__(context)
        from ...ops import require_native
        from ...ops.warp import check_parameters
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.k = int(p("quads", 4))
        self.size = int(p("image_size", 224))
        self.margin = int(p("margin", 0))
        check_parameters(self.k, (self.size, self.size), self.margin, "centre")
        self._out = {}

    def process_frame(self, stream, images, marker_corners, counts):
        from ...ops import warp as Wp
        bad = _frames_diagnostic("QuadRectify", images, Wp.MAX_SIDE)
        if bad:
            return StreamEvent.ERROR, {"diagnostic": bad}
        B = images.shape[0]
        q = marker_corners
        if not isinstance(q, torch.Tensor) or q.dtype != torch.int32 or q.dim() != 4 or q.shape[0] != B or \
                q.shape[1] < self.k or tuple(q.shape[2:]) != (4, 2) or q.device != images.device or not q.is_contiguous():
            return StreamEvent.ERROR, {"diagnostic": f"QuadRectify: marker_corners int32 [{B}, max_det >= quads = "
                                                     f"{self.k}, 4, 2] contiguous on the device required, got "
                                                     f"{tuple(getattr(q, 'shape', ()))} "
                                                     f"{getattr(q, 'dtype', type(q).__name__)}"}
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or tuple(counts.shape) != (B,) or \
                counts.device != images.device or not counts.is_contiguous():
            return StreamEvent.ERROR, {"diagnostic": f"QuadRectify: counts int32 [{B}] on the device required, got "
                                                     f"{tuple(getattr(counts, 'shape', ()))} "
                                                     f"{getattr(counts, 'dtype', type(counts).__name__)}"}
        if B * self.k > 65535:
            return StreamEvent.ERROR, {"diagnostic": f"QuadRectify: {B} frames x {self.k} quads exceed 65535 slots"}
        # one buffer pair per (shape, lane), rewritten every frame: the addresses a captured graph
        # behind this element reads stay the same
        key = (tuple(images.shape), self.lane)
        out = self._out.get(key)
        if out is None:
            out = self._out[key] = (
                torch.empty(B * self.k, self.size, self.size, 3, dtype=torch.uint8, device=self.device),
                torch.empty(B * self.k, dtype=torch.int32, device=self.device))
        crops, valid = Wp.warp_quads(images, q, counts, self.k, (self.size, self.size), self.margin, "centre",
                                     patches=out[0], valid=out[1])
        return StreamEvent.OKAY, {"crops": crops, "crops_valid": valid, "counts": counts, "images": images}


def _parse_view(view):
    """``("name", name)`` or ``("quads", [[8 ints], ...])`` (one list: every camera) of the ``view``
    parameter; ``ValueError`` for anything else."""
    from ...ops.warp import COORD_MAX, COORD_MIN, VIEWS
    if isinstance(view, str):
        if view in VIEWS:
            return "name", view
        try:
            view = json.loads(view)
        except ValueError:
            raise ValueError(f"FrameWarp: view one of {VIEWS} or eight integers required, got {view!r}") from None
    if not isinstance(view, (list, tuple)) or not view:
        raise ValueError(f"FrameWarp: view one of {VIEWS} or eight integers required, got {view!r}")
    rows = list(view) if isinstance(view[0], (list, tuple)) else [view]
    quads = []
    for row in rows:
        ok = isinstance(row, (list, tuple)) and len(row) == 8 and all(
            isinstance(v, (int, float)) and not isinstance(v, bool) and int(v) == v and COORD_MIN <= v <= COORD_MAX
            for v in row)
        if not ok:
            raise ValueError(f"FrameWarp: a view of eight integers in {COORD_MIN}..{COORD_MAX} [x0, y0, x1, y1, x2, "
                             f"y2, x3, y3] (edge coordinates) required, got {row!r}")
        quads.append([int(v) for v in row])
    return "quads", quads


class FrameWarp(GpuPipelineElement):
    lane_safe = True          # output buffers per lane

    def __init__(self, context):
        context.set_protocol("frame_warp:0")
        super().__init__(context)
        from ...ops import require_native
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.kind, self.view = _parse_view(p("view", "identity"))
        size = p("size", None)
        if isinstance(size, str):
            size = json.loads(size)
        if size is not None and not (isinstance(size, (list, tuple)) and len(size) == 2 and
                                     all(isinstance(v, int) and not isinstance(v, bool) and v >= 1 for v in size)):
            raise ValueError(f"FrameWarp: size [Ho, Wo] of two integers >= 1 required, got {size!r}")
        self.out_size = None if size is None else (int(size[0]), int(size[1]))
        self._state = {}

    def _quads(self, B, H, W):
        """``(quads [[8 ints]] * B, natural size)`` for ``B`` frames of ``H`` x ``W``, or a diagnostic."""
        from ...ops.warp import view_quad
        if self.kind == "name":
            quad, size = view_quad(self.view, H, W)
            return [[v for xy in quad for v in xy]] * B, size
        if len(self.view) not in (1, B):
            return f"FrameWarp: view lists {len(self.view)} cameras, the batch has {B} frames", None
        return (self.view * B if len(self.view) == 1 else self.view), (H, W)

    def process_frame(self, stream, images):
        from ...ops import warp as Wp
        bad = _frames_diagnostic("FrameWarp", images, Wp.MAX_SIDE)
        if bad:
            return StreamEvent.ERROR, {"diagnostic": bad}
        B, H, W = images.shape[:3]
        key = (tuple(images.shape), self.lane)
        state = self._state.get(key)
        if state is None:
            # the quad tensor and the count of ones are built once per shape
            quads, size = self._quads(B, H, W)
            if size is None:
                return StreamEvent.ERROR, {"diagnostic": quads}
            Ho, Wo = self.out_size or size
            if Wo % 4:
                return StreamEvent.ERROR, {"diagnostic": f"FrameWarp: the output width must be a multiple of 4, got "
                                                         f"{Ho} x {Wo} for {H} x {W} frames: give size"}
            if Ho > Wp.MAX_SIDE or Wo > Wp.MAX_SIDE or B > 65535:
                return StreamEvent.ERROR, {"diagnostic": f"FrameWarp: {B} frames to {Ho} x {Wo} are past the limits "
                                                         f"({Wp.MAX_SIDE} pixels a side, 65535 frames)"}
            state = self._state[key] = (
                torch.tensor(quads, dtype=torch.int32).view(B, 1, 4, 2).to(self.device),
                torch.ones(B, dtype=torch.int32).to(self.device),
                torch.empty(B, Ho, Wo, 3, dtype=torch.uint8, device=self.device),
                torch.empty(B, dtype=torch.int32, device=self.device))
        quads, count, out, valid = state
        Wp.warp_quads(images, quads, count, 1, tuple(out.shape[1:3]), 0, "edge", patches=out, valid=valid)
        return StreamEvent.OKAY, {"images": out}
