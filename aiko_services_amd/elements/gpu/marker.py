"""Square fiducial markers on the device: ArUco-style markers at any rotation and under perspective
as detector rows, with no OpenCV and no host round trip.

    "(SyntheticFrames MarkerDetector DetectionOverlay)"
        DetectionOverlay name_format: "#{i}", classes = label_mod — every marker boxed with its id

* ``MarkerDetector`` — ``images`` uint8 ``[B, H, W, 3]`` -> ``detections`` fp32 ``[B, max_det, 6]`` /
  ``counts`` int32 ``[B]`` (the ``YoloDetector``'s row format with the marker's id as the class:
  ``DetectionTracker``, ``DetectionOverlay``, ``DetectionRedact`` and ``RoiCrop`` work behind it
  unchanged), ``marker_corners`` int32 ``[B, max_det, 4, 2]`` (the quad, the marker's own top-left
  first), ``marker_ids`` int32 ``[B, max_det]`` (-1 past the count) and ``labels`` int32 ``[B *
  max_det]`` (the id modulo ``label_mod``, 0 past the count: what ``DetectionOverlay`` names);
  ``images`` passes through.  The three launches of ``marker_ops.hip``
  (:func:`~aiko_services_amd.ops.marker.detect_markers`, which states the rule).  Nothing is copied
  to the host and nothing synchronises.  Stateless: one set of buffers per (shape, lane).
* ``MarkerResults`` — the host sink: ``detections`` / ``counts`` / ``marker_corners`` / ``marker_ids``
  into pinned host memory without synchronising, emitted as one :class:`DeviceResult`;
  :func:`to_overlays` turns its result into the ``overlays`` of the host ``ArucoMarkerDetector``, so
  ``ArucoMarkerOverlay`` draws the quads behind it.

Parameters of ``MarkerDetector`` (scalars): ``aruco_tags`` (``DICT_4X4_50``; ``DICT_ARUCO_ORIGINAL``
reads the original 7 x 7 markers, every other tag the 6 x 6 16-bit payload markers, as the host
element), ``cell`` (4; 4, 8 or 16 pixels: markers need a quiet zone of ``2 * cell`` pixels), ``contrast``
(64 luma levels, 1..255), ``min_side`` (24 pixels), ``max_cand`` (32 components examined per frame, at
most 64), ``max_det`` (16 rows per frame, at most 64), ``label_mod`` (1024).
"""
from __future__ import annotations

import numpy as np
import torch

from ...gpu.element import DeviceResult, GpuPipelineElement, HostRing
from ...pipeline.stream import StreamEvent

__all__ = ["MarkerDetector", "MarkerResults", "to_overlays"]


class MarkerDetector(GpuPipelineElement):
    lane_safe = True          # output buffers per lane

    def __init__(self, context):
        context.set_protocol("marker_detector:0")
        super().__init__(context)
        from ...ops import require_native
        from ...ops.marker import check_parameters, dictionary_of
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.options = dict(dictionary=dictionary_of(p("aruco_tags", "DICT_4X4_50")), cell=int(p("cell", 4)),
                            contrast=int(p("contrast", 64)), min_side=int(p("min_side", 24)),
                            max_cand=int(p("max_cand", 32)), max_det=int(p("max_det", 16)))
        check_parameters(**self.options)
        self.label_mod = int(p("label_mod", 1024))
        if self.label_mod < 1:
            raise ValueError(f"MarkerDetector: label_mod >= 1 required, got {self.label_mod}")
        self._out = {}

    def process_frame(self, stream, images):
        from ...ops import marker as M
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[-1] != 3 or \
                images.dtype != torch.uint8 or images.device.type != "cuda" or not images.is_contiguous():
            return StreamEvent.ERROR, {"diagnostic": "MarkerDetector: images uint8 [B, H, W, 3] contiguous on the "
                                                     f"device required, got {tuple(getattr(images, 'shape', ()))} "
                                                     f"{getattr(images, 'dtype', type(images).__name__)}"}
        B, H, W = images.shape[:3]
        cell, max_det = self.options["cell"], self.options["max_det"]
        gh, gw = M.grid_shape(H, W, cell)
        if H > M.MAX_SIDE or W > M.MAX_SIDE or (gh + 2) * (gw + 2) > M.MAX_GRID:
            return StreamEvent.ERROR, {"diagnostic": f"MarkerDetector: {H} x {W} at cell {cell} is a grid of {gh} x "
                                                     f"{gw} cells, past the limits ({M.MAX_SIDE} pixels a side, (Gh + 2) "
                                                     f"(Gw + 2) <= {M.MAX_GRID}): choose a larger cell"}
        key = (tuple(images.shape), self.lane)
        out = self._out.get(key)
        if out is None:
            dev, i32 = self.device, torch.int32
            out = self._out[key] = dict(det=torch.empty(B, max_det, 6, dtype=torch.float32, device=dev),
                                        count=torch.empty(B, dtype=i32, device=dev),
                                        corners=torch.empty(B, max_det, 4, 2, dtype=i32, device=dev),
                                        ids=torch.empty(B, max_det, dtype=i32, device=dev),
                                        cands=torch.empty(B, dtype=i32, device=dev),
                                        mask=torch.empty(B, gh, gw, dtype=torch.uint8, device=dev),
                                        work=torch.empty(M.work_size(B, H, W), dtype=i32, device=dev),
                                        labels=torch.empty(B * max_det, dtype=i32, device=dev))
        labels = out["labels"]
        M.detect_markers(images, **self.options, **{k: v for k, v in out.items() if k != "labels"})
        torch.clamp(out["ids"].view(-1), min=0, out=labels)         # -1 past the count -> 0
        labels.remainder_(self.label_mod)
        return StreamEvent.OKAY, {"detections": out["det"], "counts": out["count"], "marker_corners": out["corners"],
                                  "marker_ids": out["ids"], "labels": labels, "images": images}


def to_overlays(result) -> list:
    """The ``overlays`` of the host ``ArucoMarkerDetector`` from a ``MarkerResults`` result (a
    :class:`DeviceResult`, waited for here, or its dict): per frame ``{"corners": [float32 array (1,
    4, 2), ...], "ids": int32 array (N, 1)}``."""
    host = result.wait() if hasattr(result, "wait") else result
    corners, ids, count = (host[k].numpy() for k in ("corners", "ids", "count"))
    out = []
    for b in range(count.shape[0]):
        n = int(count[b])
        out.append({"corners": [corners[b, i].astype(np.float32).reshape(1, 4, 2) for i in range(n)],
                    "ids": ids[b, :n].astype(np.int32).reshape(-1, 1)})
    return out


class MarkerResults(GpuPipelineElement):
    """``detections`` fp32 ``[B, max_det, 6]``, ``counts`` int32 ``[B]``, ``marker_corners`` int32 ``[B,
    max_det, 4, 2]`` and ``marker_ids`` int32 ``[B, max_det]`` -> ``markers``: a :class:`DeviceResult`
    of pinned host copies ``det`` / ``count`` / ``corners`` / ``ids`` and the event that completes
    them (:func:`to_overlays` makes the host element's ``overlays`` of it)."""
    lane_safe = True          # pinned host ring per lane

    def __init__(self, context):
        context.set_protocol("marker_results:0")
        super().__init__(context)
        self._rings = {}

    def process_frame(self, stream, detections, counts, marker_corners, marker_ids, t_submit=None):
        sources = (detections, counts, marker_corners, marker_ids)
        key = (tuple(detections.shape), self.lane)
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
        result = DeviceResult(dict(zip(("det", "count", "corners", "ids"), host)), ev,
                              t_submit=t_submit if isinstance(t_submit, (float, torch.Tensor)) else None)
        return StreamEvent.OKAY, {"markers": ring.bind(slot, result)}
