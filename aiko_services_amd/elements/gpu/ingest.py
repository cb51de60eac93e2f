"""Raw frames into the pipeline on the device.

    "(SyntheticFrames YuvToRgb YoloDetector DetectionOverlay)"        a decoder writing NV12 into HBM
    "(VideoReadWebcam FrameUpload YuvToRgb ...)"                      raw: true, format: yuyv

``YuvToRgb`` — ``images`` device uint8 ``[B, frame_bytes]`` (tightly packed ``nv12`` / ``i420`` /
``i444`` / ``yuyv`` frames, as ``SyntheticFrames`` or ``FrameUpload`` with a raw ``format`` emit
them) -> ``images`` uint8 ``[B, height, width, 3]`` RGB: one launch of ``yuv_ops.hip``
(:func:`~aiko_services_amd.ops.yuv.yuv_to_rgb`), device to device, no synchronisation.  Placed
after a stage cut, the hop before it carries the raw slot: 1.5 or 2 bytes per pixel, not 3.

Parameters: ``format`` (nv12), ``standard`` (bt601; ``jpeg`` for Y4M files, ``bt709`` for HD
decoder output), ``height``, ``width`` (required), ``pool`` (0).  Buffering follows
``FrameResize``: ``pool: N > 0`` converts into N FramePool slots, each held by its frame until the
frame completes and marked so that a following hop sends it without a staging copy; ``pool: 0``
uses one buffer per (batch, lane), converted into through ``run_maybe_captured``.
"""
from __future__ import annotations

import torch

from ...gpu.element import FramePool, GpuPipelineElement
from ...pipeline.stream import StreamEvent

__all__ = ["YuvToRgb"]


class YuvToRgb(GpuPipelineElement):
    lane_safe = True          # output buffers per lane, pool slots per frame

    def __init__(self, context):
        context.set_protocol("yuv_to_rgb:0")
        super().__init__(context)
        from ...ops import require_native
        from ...ops import yuv as Y
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.format = str(p("format", "nv12")).lower()
        self.standard = str(p("standard", "bt601")).lower()
        if self.standard not in Y.STANDARDS:
            raise ValueError(f"YuvToRgb: unknown standard {self.standard!r} (one of {sorted(Y.STANDARDS)})")
        height, width = p("height", None), p("width", None)
        if height is None or width is None:
            raise ValueError("YuvToRgb: height and width parameters required")
        self.height, self.width = int(height), int(width)
        self.frame_bytes = Y.frame_bytes(self.format, self.height, self.width)   # unknown format: ValueError
        self.pool_slots = int(p("pool", 0))
        self._out = {}
        self._pools = {}

    def _convert(self, raw, out):
        from ...ops import yuv as Y
        return Y.yuv_to_rgb(raw, self.height, self.width, self.format, self.standard, out=out)

    def process_frame(self, stream, images):
        if images.dim() != 2 or images.shape[1] != self.frame_bytes:
            raise ValueError(f"YuvToRgb: a {self.format} frame of {self.height} x {self.width} has "
                             f"{self.frame_bytes} bytes, got images {tuple(images.shape)}")
        B = images.shape[0]
        shape = (B, self.height, self.width, 3)
        if self.pool_slots > 0:
            pool = self._pools.get(B)
            if pool is None:
                pool = self._pools[B] = FramePool(self.pool_slots, B * self.height * self.width * 3,
                                                  device=self.device)
            slot = pool.acquire(30.0)
            if slot >= 0:
                out = pool.view(slot, shape, torch.uint8)
                self.hold_for_frame(pool, slot)
                from ...parallel.hop import mark_frame_held
                # the output changes with the slot: a direct launch (a single kernel either way)
                return StreamEvent.OKAY, {"images": mark_frame_held(self._convert(images, out))}
        out = self._out.get((B, self.lane))
        if out is None:
            out = self._out[(B, self.lane)] = torch.empty(shape, dtype=torch.uint8, device=self.device)
        rgb = self.run_maybe_captured(("yuv", B), lambda raw: self._convert(raw, out), images)
        return StreamEvent.OKAY, {"images": rgb}
