"""Antialiased resize on the device: frames to any size with the host path's picture.

    "(SyntheticFrames YoloDetector DetectionOverlay FrameScale JpegEncode JpegResults)"

* ``FrameScale`` — ``images`` uint8 ``[B, H, W, 3]`` -> ``images`` uint8 ``[B, height, width, 3]``:
  the part of every frame inside ``box`` (default: all of it) scaled with ``filter``, separable and
  in fixed point (``scale_ops.hip``).  Every byte is what Pillow's ``Image.resize`` gives with the
  same filter and box, so thumbnails, classifier inputs and reduced camera frames made on the device
  equal the ones the host elements make; the rule is stated in :mod:`~aiko_services_amd.ops.scale`.
  ``JpegEncode``, ``RgbToYuv``, ``FrameDownload`` and the models take the result as any batch.

Nothing is copied to the host and nothing synchronises, so ``FrameScale`` replays inside hipGraphs
and frame lanes: the coefficient tables of a (shape, size, filter, box) are made and uploaded once,
on the first frame of that shape.  It is stateless; its output is a buffer of its own per (shape,
lane).  The same size with no box passes the batch through.

Parameters (scalars): ``width``, ``height`` (required), ``filter`` (``bicubic``, Pillow's default;
one of ``box``, ``bilinear``, ``hamming``, ``bicubic``, ``lanczos``) and ``box``, the JSON text of
four numbers ``"[left, top, right, bottom]"`` in pixels, each a multiple of 1/16: other values do not
reproduce between float32 and float64 and are refused.
"""
from __future__ import annotations

import json

import torch

from ...gpu.element import GpuPipelineElement
from ...pipeline.stream import StreamEvent

__all__ = ["FrameScale"]


class FrameScale(GpuPipelineElement):
    lane_safe = True          # stateless; output buffers per lane

    def __init__(self, context):
        context.set_protocol("frame_scale:0")
        super().__init__(context)
        from ...ops import require_native
        from ...ops import scale as Sc
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        width, height = p("width", None), p("height", None)
        if width is None or height is None:
            raise ValueError("FrameScale: width and height are required")
        try:
            self.size = Sc.check_size((int(height), int(width)))
            self.filter = str(p("filter", "bicubic"))
            if self.filter not in Sc.FILTERS:
                raise ValueError(f"filter one of {sorted(Sc.FILTERS)} required, got {self.filter!r}")
            box = p("box", None)
            if isinstance(box, str):                          # a parameter set as text
                try:
                    box = json.loads(box)
                except ValueError:
                    raise ValueError(f"box = JSON text of four numbers required, got {box!r}") from None
            self.box = None if box is None else Sc.box_from_pixels(box)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"FrameScale: {exc}") from None
        self._out = {}

    def process_frame(self, stream, images):
        from ...ops import scale as Sc
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or \
                images.shape[3] != 3 or images.device.type != "cuda" or not images.is_contiguous():
            return StreamEvent.ERROR, {"diagnostic": "FrameScale: images uint8 [B, H, W, 3] contiguous on the device "
                                                     f"required, got {tuple(getattr(images, 'shape', ()))} "
                                                     f"{getattr(images, 'dtype', type(images).__name__)}"}
        H, W = int(images.shape[1]), int(images.shape[2])
        try:
            plan = Sc.scale_plan(H, W, self.size, self.filter, self.box, images.device)
        except ValueError as exc:                              # a box outside these frames, a ratio past MAX_TAPS
            return StreamEvent.ERROR, {"diagnostic": f"FrameScale: {exc}"}
        if plan.hb is None and plan.vb is None:
            return StreamEvent.OKAY, {"images": images}
        # one buffer per (shape, lane), rewritten every frame: a stable address for whatever reads it next
        key = (tuple(images.shape), self.lane)
        out = self._out.get(key)
        if out is None:
            out = self._out[key] = torch.empty(images.shape[0], *self.size, 3, dtype=torch.uint8, device=images.device)
        try:
            Sc.scale_frames(images, self.size, self.filter, self.box, out=out)
        except ValueError as exc:
            return StreamEvent.ERROR, {"diagnostic": f"FrameScale: {exc}"}
        return StreamEvent.OKAY, {"images": out}
