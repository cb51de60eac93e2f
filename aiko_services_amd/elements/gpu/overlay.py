"""Annotated frames on the device: the last stage of a detect(-then-classify) pipeline.

    "(SyntheticFrames YoloDetector (RoiCrop ResNet50Classifier (crops: images)) DetectionOverlay)"

``DetectionOverlay`` — ``images`` uint8 ``[B, H, W, 3]`` + the ``YoloDetector``'s ``detections``
``[B, max_det, 6]`` / ``counts`` ``[B]`` and, optionally, a classifier's ``logits``
``[B*rois, C]`` over the crops of ``RoiCrop`` -> ``images``: the frames with the first ``rois``
boxes of every frame outlined and labelled.  One HIP kernel (``overlay_ops.hip``) reads rows and
counts on the device; with ``logits`` the top-1 class and probability of every ROI slot come from
``softmax_topk`` into the element's own buffers and replace the detector's class and score.
Instead of ``logits`` the element takes ``labels``, int32 ``[B*rois]``: the class of every ROI slot
as it stands (the ``DetectionTracker``'s ``labels`` = track id modulo ``label_mod``; the score stays
the detector's).
Nothing is copied to the host and nothing synchronises, so the element replays inside hipGraphs
and frame lanes.  The output is a buffer of the element's own per (shape, lane), never the input:
the input slots belong to the frame pool and other elements may still read them.

Parameters: ``rois`` (8; must equal ``RoiCrop``'s when ``logits`` are used), ``margin`` (0.0; the
drawn rect equals ``RoiCrop``'s ``rois`` for the same margin), ``thickness`` (2), ``text_scale``
(1), ``show_score`` (true), ``names`` (a list, or the path of a text file with one name per line;
default ``name_format`` filled in for each of the ``classes`` classes), ``name_format``
(``"class_{i}"``; ``"#{i}"`` with a tracker's ``labels`` and ``classes`` = its ``label_mod`` names a
box by its track, in the colour ``palette[id % P]``, the same in every frame), ``classes`` (the
width of ``logits``, or 80 without them), ``name_width`` (16 characters kept per name), ``palette``
(a list of RGB triples; default ``ops.overlay.default_palette(20)``).
"""
from __future__ import annotations

import torch

from ...gpu.element import GpuPipelineElement
from ...pipeline.stream import StreamEvent

__all__ = ["DetectionOverlay"]


def _flag(value) -> bool:
    return str(value).lower() in ("true", "1", "yes")


class DetectionOverlay(GpuPipelineElement):
    lane_safe = True          # output buffers per lane

    def __init__(self, context):
        context.set_protocol("detection_overlay:0")
        super().__init__(context)
        from ...ops import require_native
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.k = int(p("rois", 8))
        self.margin = float(p("margin", 0.0))
        self.thickness = int(p("thickness", 2))
        self.text_scale = int(p("text_scale", 1))
        self.show_score = _flag(p("show_score", True))
        self.name_width = int(p("name_width", 16))
        self._names_param = p("names", None)
        self._name_format = str(p("name_format", "class_{i}"))
        self._classes = p("classes", None)
        self._palette_param = p("palette", None)
        self._tables = None
        self._out = {}

    def _ensure_tables(self, logits):
        if self._tables is not None:
            return self._tables
        from ...ops import overlay as O
        names = self._names_param
        if isinstance(names, str):
            with open(names, encoding="ascii") as f:
                names = [line.rstrip("\r\n") for line in f]
        if names is None:
            classes = int(self._classes) if self._classes is not None else \
                (logits.shape[1] if logits is not None else 80)
            names = [self._name_format.format(i=i) for i in range(classes)]
        palette = O.default_palette(20) if self._palette_param is None else \
            torch.tensor(self._palette_param, dtype=torch.uint8).reshape(-1, 3)
        font, gw = O.default_font()
        self._tables = (O.pack_names(list(names), self.name_width).to(self.device), font.to(self.device),
                        palette.to(self.device), gw)
        return self._tables

    def process_frame(self, stream, images, detections, counts, logits=None, labels=None):
        from ...ops import overlay as O
        from ...ops.vision import softmax_topk
        names, font, palette, gw = self._ensure_tables(logits)
        B = images.shape[0]
        if logits is not None and logits.shape[0] != B * self.k:
            return StreamEvent.ERROR, {"diagnostic": f"DetectionOverlay: {logits.shape[0]} logit rows for "
                                                     f"{B} frames x rois = {self.k}: rois must equal RoiCrop's"}
        if labels is not None:
            if logits is not None:
                return StreamEvent.ERROR, {"diagnostic": "DetectionOverlay: labels and logits both given: the class "
                                                         "of a slot comes from one of them"}
            if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or labels.numel() != B * self.k:
                return StreamEvent.ERROR, {"diagnostic": f"DetectionOverlay: labels int32 [{B} frames x rois = "
                                                         f"{self.k}] required, got {tuple(getattr(labels, 'shape', ()))}"}
            labels = labels.view(-1)
        # one set of buffers per (shape, lane), rewritten every frame: stable addresses for
        # whatever reads the annotated frames next
        key = (tuple(images.shape), None if logits is None else tuple(logits.shape), self.lane)
        buf = self._out.get(key)
        if buf is None:
            top = None
            if logits is not None:
                top = (torch.empty(B * self.k, 1, dtype=torch.float32, device=self.device),
                       torch.empty(B * self.k, 1, dtype=torch.int32, device=self.device))
            buf = self._out[key] = (torch.empty_like(images), top)
        out, top = buf
        scores = None
        if logits is not None:
            prob, index = softmax_topk(logits, 1, prob=top[0], index=top[1])
            labels, scores = index.view(-1), prob.view(-1)
        O.draw_detections(images, detections, counts, self.k, names, font, palette, labels=labels, scores=scores,
                          thickness=self.thickness, text_scale=self.text_scale, margin=self.margin,
                          show_score=self.show_score, glyph_width=gw, out=out)
        return StreamEvent.OKAY, {"images": out}
