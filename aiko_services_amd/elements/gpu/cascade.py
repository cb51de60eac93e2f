"""Detect-then-classify on the device: a secondary classifier over the detector's boxes (the shape
of the reference's face example: detect -> crop -> represent).

    "(SyntheticFrames YoloDetector (RoiCrop ResNet50Classifier (crops: images)) ClassifierTopK RoiResults)"

* ``RoiCrop`` — ``images`` uint8 ``[B, H, W, 3]`` + the ``YoloDetector``'s ``detections``
  ``[B, max_det, 6]`` / ``counts`` ``[B]`` -> ``crops`` uint8 ``[B*rois, S, S, 3]`` (the first
  ``rois`` boxes of every frame in score order, resized to ``image_size``; zeros where a frame has
  fewer) and ``rois`` int32 ``[B*rois, 4]`` (the frame rect of each crop, zeros where unused).  One
  HIP kernel (``roi_ops.hip``) reads the rows and the counts on the device: nothing is copied to
  the host and nothing synchronises, so the element replays inside hipGraphs and frame lanes.
  The ``(crops: images)`` mapping on the edge RoiCrop -> ResNet50Classifier feeds it the crops.
* ``RoiResults`` — the detection side's result sink: ``detections`` / ``counts`` / ``rois`` into
  pinned host memory without synchronising, emitted as one :class:`DeviceResult`.
"""
from __future__ import annotations

import torch

from ...gpu.element import DeviceResult, GpuPipelineElement, HostRing
from ...pipeline.stream import StreamEvent

__all__ = ["RoiCrop", "RoiResults"]


class RoiCrop(GpuPipelineElement):
    lane_safe = True          # output buffers per lane

    def __init__(self, context):
        context.set_protocol("roi_crop:0")
        super().__init__(context)
        from ...ops import require_native
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.k = int(p("rois", 8))
        self.size = int(p("image_size", 224))
        self.margin = float(p("margin", 0.0))
        self._out = {}

    def process_frame(self, stream, images, detections, counts):
        from ...ops import roi as R
        # one buffer pair per (shape, lane), rewritten every frame: the addresses the classifier's
        # captured graph reads stay the same
        key = (tuple(images.shape), self.lane)
        out = self._out.get(key)
        if out is None:
            n = images.shape[0] * self.k
            out = self._out[key] = (
                torch.empty(n, self.size, self.size, 3, dtype=torch.uint8, device=self.device),
                torch.empty(n, 4, dtype=torch.int32, device=self.device))
        crops, rois = R.roi_crop(images, detections, counts, self.k, (self.size, self.size), self.margin,
                                 crops=out[0], rois=out[1])
        return StreamEvent.OKAY, {"crops": crops, "rois": rois, "counts": counts}


class RoiResults(GpuPipelineElement):
    """``detections`` fp32 ``[B, max_det, 6]``, ``counts`` int32 ``[B]`` and ``rois`` int32
    ``[B*K, 4]`` -> ``regions``: a :class:`DeviceResult` of pinned host copies ``det`` / ``count``
    / ``rois`` and the event that completes them."""
    lane_safe = True          # pinned host ring per lane

    def __init__(self, context):
        context.set_protocol("roi_results:0")
        super().__init__(context)
        self._rings = {}

    def process_frame(self, stream, detections, counts, rois, t_submit=None):
        key = (tuple(detections.shape), tuple(rois.shape), self.lane)
        ring = self._rings.get(key)
        if ring is None:
            pin = self.device.type == "cuda"
            specs = [(tuple(t.shape), t.dtype) for t in (detections, counts, rois)]
            ring = self._rings[key] = HostRing(
                lambda: tuple(torch.empty(s, dtype=d, pin_memory=pin) for s, d in specs), 8)
        slot, host = ring.acquire()
        for dst, src in zip(host, (detections, counts, rois)):
            dst.copy_(src, non_blocking=True)
        ev = None
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
        result = DeviceResult(dict(zip(("det", "count", "rois"), host)), ev,
                              t_submit=t_submit if isinstance(t_submit, (float, torch.Tensor)) else None)
        return StreamEvent.OKAY, {"regions": ring.bind(slot, result)}
