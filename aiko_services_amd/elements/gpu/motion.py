"""Motion detection on the device: moving regions of a fixed camera's view as detector rows, with
no neural network in the graph.

    "(SyntheticFrames MotionDetector DetectionTracker DetectionOverlay)"
        DetectionOverlay name_format: "#{i}" — every moving region numbered across frames and drawn

* ``MotionDetector`` — ``images`` uint8 ``[B, H, W, 3]`` -> ``detections`` fp32 ``[B, max_det, 6]`` /
  ``counts`` int32 ``[B]`` (the ``YoloDetector``'s row format: ``DetectionTracker``,
  ``DetectionOverlay``, ``DetectionRedact`` and ``RoiCrop`` work behind it unchanged), ``motion_mask``
  uint8 ``[B, Gh, Gw]`` (1 where a cell moves) and ``motion_cells`` int32 ``[B]``; ``images`` passes
  through.  Batch row ``b`` is camera ``b`` and successive pipeline frames are successive instants:
  the row's background of cell levels stays in HBM and the two launches of ``motion_ops.hip``
  (:func:`~aiko_services_amd.ops.motion.motion_detect`, which states the rule) advance it.  Nothing
  is copied to the host and nothing synchronises.
* ``MotionResults`` — the host sink: ``detections`` / ``counts`` / ``motion_mask`` / ``motion_cells``
  into pinned host memory without synchronising, emitted as one :class:`DeviceResult`.

Parameters of ``MotionDetector`` (scalars): ``cell`` (16; 8, 16 or 32 pixels), ``threshold`` (12 luma
levels, 0..255), ``learn_shift`` (4: the background moves 1/16 of the way per frame, 0..8),
``learn_moving`` (true: moving cells are learnt too, so a parked car fades into the background),
``warmup`` (1 frame before anything is reported), ``min_cells`` (2: smaller regions are dropped),
``max_det`` (16 rows per frame, at most 64).

Frame k reads the state frame k-1 wrote and writes its own, into set k % R of a ring of R =
max(2, lanes + 1) (state, outputs) sets, and waits for frame k-1's launches first (an event chain
across the lane streams): ``DetectionTracker``'s scheme, which argues why a set is free when it is
written again.  The state starts empty and is reset when ``B``, ``H``, ``W`` or ``cell`` changes.
"""
from __future__ import annotations

import torch

from ...gpu.element import DeviceResult, GpuPipelineElement, HostRing
from ...pipeline.stream import StreamEvent

__all__ = ["MotionDetector", "MotionResults"]


def _flag(value) -> bool:
    return str(value).lower() in ("true", "1", "yes")


class MotionDetector(GpuPipelineElement):
    lane_safe = True          # state and output ring, ordered by an event chain

    def __init__(self, context):
        context.set_protocol("motion_detector:0")
        super().__init__(context)
        from ...ops import require_native
        from ...ops.motion import check_parameters
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.options = dict(cell=int(p("cell", 16)), threshold=int(p("threshold", 12)),
                            learn_shift=int(p("learn_shift", 4)), learn_moving=_flag(p("learn_moving", True)),
                            warmup=int(p("warmup", 1)), min_cells=int(p("min_cells", 2)),
                            max_det=int(p("max_det", 16)))
        check_parameters(**{k: v for k, v in self.options.items() if k != "learn_moving"})
        self._ring = None
        self._key = None
        self._cur = 0
        self._last = None

    def process_frame(self, stream, images):
        from ...ops import motion as M
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[-1] != 3 or \
                images.dtype != torch.uint8 or images.device.type != "cuda" or not images.is_contiguous():
            return StreamEvent.ERROR, {"diagnostic": "MotionDetector: images uint8 [B, H, W, 3] contiguous on the "
                                                     f"device required, got {tuple(getattr(images, 'shape', ()))} "
                                                     f"{getattr(images, 'dtype', type(images).__name__)}"}
        B, H, W = images.shape[:3]
        cell, max_det = self.options["cell"], self.options["max_det"]
        gh, gw = M.grid_shape(H, W, cell)
        if gh > 255 or gw > 255 or gh * gw > 16384:
            return StreamEvent.ERROR, {"diagnostic": f"MotionDetector: {H} x {W} at cell {cell} is a grid of {gh} x "
                                                     f"{gw} cells, past the limits (255 x 255, 16384 cells)"}
        lanes = getattr(self.pipeline, "_lanes_cfg", (1, None))[0] if self.pipeline is not None else 1
        R = max(2, lanes + 1)
        key = (R, B, H, W, cell)
        ring = self._ring
        if ring is None or self._key != key:
            dev = self.device
            ring = self._ring = [(M.new_state(B, H, W, cell, dev),
                                  (torch.empty(B, max_det, 6, dtype=torch.float32, device=dev),
                                   torch.empty(B, dtype=torch.int32, device=dev),
                                   torch.empty(B, gh, gw, dtype=torch.uint8, device=dev),
                                   torch.empty(B, dtype=torch.int32, device=dev))) for _ in range(R)]
            self._key = key
            self._cur = 0
        state = ring[self._cur][0]
        self._cur = (self._cur + 1) % R
        state_out, (det, count, mask, cells) = ring[self._cur]
        if self._last is not None:
            torch.cuda.current_stream(self.device).wait_event(self._last)
        M.motion_detect(images, state, state_out=state_out, det=det, count=count, mask=mask, cells=cells,
                        **self.options)
        self._last = torch.cuda.Event()
        self._last.record()
        return StreamEvent.OKAY, {"detections": det, "counts": count, "motion_mask": mask, "motion_cells": cells,
                                  "images": images}


class MotionResults(GpuPipelineElement):
    """``detections`` fp32 ``[B, max_det, 6]``, ``counts`` int32 ``[B]``, ``motion_mask`` uint8 ``[B,
    Gh, Gw]`` and ``motion_cells`` int32 ``[B]`` -> ``motion``: a :class:`DeviceResult` of pinned host
    copies ``det`` / ``count`` / ``mask`` / ``cells`` and the event that completes them."""
    lane_safe = True          # pinned host ring per lane

    def __init__(self, context):
        context.set_protocol("motion_results:0")
        super().__init__(context)
        self._rings = {}

    def process_frame(self, stream, detections, counts, motion_mask, motion_cells, t_submit=None):
        sources = (detections, counts, motion_mask, motion_cells)
        key = (tuple(detections.shape), tuple(motion_mask.shape), self.lane)
        ring = self._rings.get(key)
        if ring is None:
            pin = self.device.type == "cuda"
            specs = [(tuple(t.shape), t.dtype) for t in sources]
            ring = self._rings[key] = HostRing(
                lambda: tuple(torch.empty(s, dtype=d, pin_memory=pin) for s, d in specs), 8)
        slot, host = ring.acquire()
        for dst, src in zip(host, sources):
            dst.copy_(src, non_blocking=True)
        ev = None
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
        result = DeviceResult(dict(zip(("det", "count", "mask", "cells"), host)), ev,
                              t_submit=t_submit if isinstance(t_submit, (float, torch.Tensor)) else None)
        return StreamEvent.OKAY, {"motion": ring.bind(slot, result)}
