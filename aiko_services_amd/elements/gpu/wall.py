"""The camera wall on the device: every camera of a batch in one picture.

    "(SyntheticFrames (MotionDetector DetectionOverlay FrameWall (motion_cells: scores)) JpegEncode JpegResults)"

* ``FrameWall`` — ``images`` uint8 ``[B, H, W, 3]`` (batch row ``b`` is camera ``b``) and,
  optionally, ``scores`` int32 ``[B]`` -> ``images`` uint8 ``[pages, Hw, Ww, 3]``, the wall, and
  ``wall_sources`` int32 ``[pages, rows*cols]``, the camera of every tile or -1.  ``scores`` is what
  a graph mapping hands it: ``(counts: scores)`` behind a ``YoloDetector``, ``(motion_cells:
  scores)`` behind a ``MotionDetector``.  Two HIP launches (``wall_ops.hip``) pick the cameras and
  compose the tiles on the device; the rule is stated in :mod:`~aiko_services_amd.ops.wall`.
  ``JpegEncode``, ``RgbToYuv`` and ``FrameDownload`` take the wall as they take any batch.
* ``WallResults`` — the host sink: ``wall_sources`` into pinned host memory without
  synchronising, emitted as one :class:`DeviceResult`.

Nothing is copied to the host and nothing synchronises, so ``FrameWall`` replays inside hipGraphs
and frame lanes.  It is stateless; its outputs are buffers of its own per (shape, lane).

Parameters of ``FrameWall`` (scalars): ``rows`` (4), ``cols`` (4), ``tile_height`` / ``tile_width``
(default ``H // d`` / ``W // d`` with ``d = max(rows, cols)``), ``gap`` (0), ``pages`` (1),
``order`` (``index`` or ``score``), ``min_score`` (1), ``ring`` (0), ``label_scale`` (1; 0 = no
numbers), ``label_base`` (0).  The colours ``background`` ([0, 0, 0]), ``alert`` ([255, 0, 0]),
``label_fg`` ([255, 255, 255]) and ``label_bg`` ([0, 0, 0]) are RGB; a pipeline definition's
parameters are scalars, so there they are written as JSON text: ``"alert": "[255, 160, 0]"``.
"""
from __future__ import annotations

import json

import torch

from ...gpu.element import DeviceResult, GpuPipelineElement, HostRing
from ...pipeline.stream import StreamEvent

__all__ = ["FrameWall", "WallResults"]


class FrameWall(GpuPipelineElement):
    lane_safe = True          # stateless; output buffers per lane

    def __init__(self, context):
        context.set_protocol("frame_wall:0")
        super().__init__(context)
        from ...ops import require_native
        from ...ops import wall as Wl
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        as_list = lambda v: json.loads(v) if isinstance(v, str) else v  # noqa: E731  (a parameter set as text)
        self.rows, self.cols = int(p("rows", 4)), int(p("cols", 4))
        th, tw = p("tile_height", None), p("tile_width", None)
        if (th is None) != (tw is None):
            raise ValueError("FrameWall: tile_height and tile_width are given together or not at all")
        self.tile = None if th is None else (int(th), int(tw))
        self.order = str(p("order", "index"))
        self.options = dict(gap=int(p("gap", 0)), pages=int(p("pages", 1)), min_score=int(p("min_score", 1)),
                            ring=int(p("ring", 0)), label_scale=int(p("label_scale", 1)),
                            label_base=int(p("label_base", 0)))
        for name, default in (("background", [0, 0, 0]), ("alert", [255, 0, 0]), ("label_fg", [255, 255, 255]),
                              ("label_bg", [0, 0, 0])):
            self.options[name] = tuple(as_list(p(name, default)))
        try:                  # what does not depend on the frames; ring against the tile once they are known
            Wl.check_parameters(rows=self.rows, cols=self.cols, tile=self.tile or (1 << 23, 1 << 23), order=self.order,
                                **self.options)
        except ValueError as exc:
            raise ValueError(f"FrameWall: {exc}") from None
        self._out = {}

    def process_frame(self, stream, images, scores=None):
        from ...ops import wall as Wl
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or \
                images.shape[3] != 3 or images.device.type != "cuda" or not images.is_contiguous():
            return StreamEvent.ERROR, {"diagnostic": "FrameWall: images uint8 [B, H, W, 3] contiguous on the device "
                                                     f"required, got {tuple(getattr(images, 'shape', ()))} "
                                                     f"{getattr(images, 'dtype', type(images).__name__)}"}
        B, H, W = images.shape[:3]
        if scores is not None and (not isinstance(scores, torch.Tensor) or scores.dtype != torch.int32 or
                                   tuple(scores.shape) != (B,)):
            return StreamEvent.ERROR, {"diagnostic": f"FrameWall: scores int32 [{B}] required, got "
                                                     f"{tuple(getattr(scores, 'shape', ()))}"}
        if scores is None and self.order == "score":
            return StreamEvent.ERROR, {"diagnostic": "FrameWall: order 'score' requires scores (a graph mapping such "
                                                     "as (counts: scores))"}
        tile = self.tile or Wl.default_tile(H, W, self.rows, self.cols)
        try:
            Wl.check_parameters(rows=self.rows, cols=self.cols, tile=tile, order=self.order, frame=(H, W),
                                **self.options)
        except ValueError as exc:
            return StreamEvent.ERROR, {"diagnostic": f"FrameWall: {exc}"}
        if self.order == "score" and B > Wl.MAX_RANKED:
            return StreamEvent.ERROR, {"diagnostic": f"FrameWall: score order ranks at most {Wl.MAX_RANKED} cameras, "
                                                     f"got {B}"}
        # one pair of buffers per (shape, lane), rewritten every frame: a stable address for
        # whatever reads the wall next
        key = (tuple(images.shape), self.lane)
        bufs = self._out.get(key)
        if bufs is None:
            pages = self.options["pages"]
            bufs = self._out[key] = (
                torch.empty(pages, *Wl.wall_shape(self.rows, self.cols, tile, self.options["gap"]), 3,
                            dtype=torch.uint8, device=images.device),
                torch.empty(pages, self.rows * self.cols, dtype=torch.int32, device=images.device))
        wall, source = bufs
        Wl.frame_wall(images, scores, rows=self.rows, cols=self.cols, tile=tile, order=self.order, out=wall,
                      source=source, **self.options)
        return StreamEvent.OKAY, {"images": wall, "wall_sources": source}


class WallResults(GpuPipelineElement):
    """``wall_sources`` int32 ``[pages, rows*cols]`` -> ``wall``: a :class:`DeviceResult` of the
    pinned host copy ``sources`` and the event that completes it."""
    lane_safe = True          # pinned host ring per lane

    def __init__(self, context):
        context.set_protocol("wall_results:0")
        super().__init__(context)
        self._rings = {}

    def process_frame(self, stream, wall_sources, t_submit=None):
        key = (tuple(wall_sources.shape), self.lane)
        ring = self._rings.get(key)
        if ring is None:
            pin = self.device.type == "cuda"
            shape, dtype = tuple(wall_sources.shape), wall_sources.dtype
            ring = self._rings[key] = HostRing(lambda: (torch.empty(shape, dtype=dtype, pin_memory=pin),), 8)
        slot, host = ring.acquire()
        host[0].copy_(wall_sources, non_blocking=True)
        ev = None
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
        result = DeviceResult({"sources": host[0]}, ev,
                              t_submit=t_submit if isinstance(t_submit, (float, torch.Tensor)) else None)
        return StreamEvent.OKAY, {"wall": ring.bind(slot, result)}
