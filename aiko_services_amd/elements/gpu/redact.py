"""Redacted frames on the device: what must not be seen is hidden before a frame leaves the GPU.

    "(SyntheticFrames YoloDetector DetectionRedact DetectionOverlay RgbToYuv)"

``DetectionRedact`` — ``images`` uint8 ``[B, H, W, 3]`` + the ``YoloDetector``'s ``detections``
``[B, max_det, 6]`` / ``counts`` ``[B]`` and, optionally, ``labels`` int32 ``[B*rois]`` ->
``images``: the frames with the first ``rois`` boxes of every frame pixelated (a mosaic of
``block`` x ``block`` cells anchored at the frame's origin) or filled with one colour, for the
classes listed in ``classes``.  One HIP kernel (``redact_ops.hip``) reads rows and counts on the
device; the rule is stated in :mod:`~aiko_services_amd.ops.redact`.  ``detections`` and ``counts``
pass through untouched, so a ``DetectionOverlay`` behind this element draws on the redacted frames.

``labels`` is a class per ROI slot as it stands, e.g. a cascade classifier's top-1 over the crops
of ``RoiCrop``; it replaces the detector's class in the selection.  A ``DetectionTracker``'s
``labels`` are track ids modulo ``label_mod``, not classes: do not connect them here.

Nothing is copied to the host and nothing synchronises, so the element replays inside hipGraphs
and frame lanes.  The output is a buffer of the element's own per (shape, lane), never the input:
the input slots belong to the frame pool and other elements may still read them.

Parameters: ``rois`` (8), ``margin`` (0.0; the redacted rect equals ``RoiCrop``'s ``rois`` and
``DetectionOverlay``'s outline for the same margin), ``mode`` (``pixelate`` or ``fill``), ``block``
(16; one of 4, 8, 16, 32), ``fill`` ([0, 0, 0], RGB), ``classes`` (a list of class ids; default:
every class), ``class_count`` (the length of the selection table: 80, or ``max(classes) + 1`` if
that is larger; a class at or past it is never redacted).  A pipeline definition's parameters are
scalars, so there ``fill`` and ``classes`` are written as JSON text: ``"classes": "[0, 2]"``.
"""
from __future__ import annotations

import json

import torch

from ...gpu.element import GpuPipelineElement
from ...pipeline.stream import StreamEvent

__all__ = ["DetectionRedact"]


class DetectionRedact(GpuPipelineElement):
    lane_safe = True          # output buffers per lane

    def __init__(self, context):
        context.set_protocol("detection_redact:0")
        super().__init__(context)
        from ...ops import require_native
        from ...ops import redact as R
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.k = int(p("rois", 8))
        self.margin = float(p("margin", 0.0))
        self.mode = str(p("mode", "pixelate"))
        self.block = int(p("block", 16))
        as_list = lambda v: json.loads(v) if isinstance(v, str) else v  # noqa: E731  (a parameter set as text)
        self.fill = tuple(int(c) for c in as_list(p("fill", [0, 0, 0])))
        classes = as_list(p("classes", None))
        if self.k < 1:
            raise ValueError(f"DetectionRedact: rois >= 1 required, got {self.k}")
        if not (0.0 <= self.margin <= 3.0e38):
            raise ValueError(f"DetectionRedact: a finite margin >= 0 required, got {self.margin}")
        if self.mode not in R.MODES:
            raise ValueError(f"DetectionRedact: mode one of {sorted(R.MODES)} required, got {self.mode!r}")
        if self.block not in R.BLOCKS:
            raise ValueError(f"DetectionRedact: block one of {list(R.BLOCKS)} required, got {self.block}")
        if len(self.fill) != 3 or not all(0 <= c <= 255 for c in self.fill):
            raise ValueError(f"DetectionRedact: fill = [R, G, B] with components 0..255 required, got {self.fill}")
        self._select_host = None                               # every class
        if classes is not None:
            classes = [int(c) for c in classes]
            n = max(int(p("class_count", 80)), max(classes, default=-1) + 1)
            self._select_host = R.class_select(classes, n)
        self._select = None
        self._out = {}

    def process_frame(self, stream, images, detections, counts, labels=None):
        from ...ops import redact as R
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or \
                images.shape[3] != 3:
            return StreamEvent.ERROR, {"diagnostic": f"DetectionRedact: images uint8 [B, H, W, 3] required, got "
                                                     f"{tuple(getattr(images, 'shape', ()))}"}
        B = images.shape[0]
        if not isinstance(detections, torch.Tensor) or detections.dim() != 3 or detections.shape[0] != B or \
                detections.shape[2] != 6 or detections.shape[1] < self.k:
            return StreamEvent.ERROR, {"diagnostic": f"DetectionRedact: detections [{B}, max_det >= rois = {self.k}, 6] "
                                                     f"required, got {tuple(getattr(detections, 'shape', ()))}"}
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or tuple(counts.shape) != (B,):
            return StreamEvent.ERROR, {"diagnostic": f"DetectionRedact: counts int32 [{B}] required, got "
                                                     f"{tuple(getattr(counts, 'shape', ()))}"}
        if labels is not None:
            if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or labels.numel() != B * self.k:
                return StreamEvent.ERROR, {"diagnostic": f"DetectionRedact: labels int32 [{B} frames x rois = "
                                                         f"{self.k}] required, got {tuple(getattr(labels, 'shape', ()))}"}
            labels = labels.view(-1)
        if self._select_host is not None and self._select is None:
            self._select = self._select_host.to(self.device)
        # one buffer per (shape, lane), rewritten every frame: a stable address for whatever reads
        # the redacted frames next
        key = (tuple(images.shape), self.lane)
        out = self._out.get(key)
        if out is None:
            out = self._out[key] = torch.empty_like(images)
        R.redact_detections(images, detections, counts, self.k, mode=self.mode, block=self.block, fill=self.fill,
                            margin=self.margin, select=self._select, labels=labels, out=out)
        return StreamEvent.OKAY, {"images": out, "detections": detections, "counts": counts}
