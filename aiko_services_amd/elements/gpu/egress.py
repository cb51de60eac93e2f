"""Raw frames out of the pipeline on the device, and device frames back to host sinks.

    "(SyntheticFrames YuvToRgb YoloDetector DetectionOverlay RgbToYuv)"    NV12 in, annotated NV12 out
    "(... DetectionOverlay RgbToYuv FrameDownload VideoWriteFile)"          raw: true, format: i420

``RgbToYuv`` — ``images`` device uint8 ``[B, H, W, 3]`` RGB -> ``images`` uint8 ``[B, frame_bytes]``
(tightly packed ``nv12`` / ``i420`` / ``i444`` / ``yuyv`` frames): one launch of ``yuv_out_ops.hip``
(:func:`~aiko_services_amd.ops.yuv.rgb_to_yuv`), device to device, no synchronisation.  The inverse
of ``YuvToRgb``: what a hardware encoder (NV12), a Y4M file (planar) or a camera loop-back (YUYV)
takes.  Placed before a stage cut, the hop after it carries 1.5 or 2 bytes per pixel, not 3.

Parameters: ``format`` (nv12), ``standard`` (bt601; ``jpeg`` for Y4M files, ``bt709`` for HD
encoders), ``pool`` (0).  Buffering is ``YuvToRgb``'s: ``pool: N > 0`` converts into N FramePool
slots, each held by its frame until the frame completes and marked so that a following hop sends
it without a staging copy; ``pool: 0`` uses one buffer per (batch, lane), converted into through
``run_maybe_captured``.

``FrameDownload`` — the counterpart of ``FrameUpload``: device ``images`` of any uint8 shape ``[B,
...]`` are copied into a pinned host set (``HostRing``) without blocking the stream; the element
waits for that copy's event only and emits ``images`` as a list of B numpy arrays, views of the
pinned set, which is reused once the consumer has dropped them.  Host sinks (``VideoWriteFile``,
``ImageWriteFile``, ``VideoShow``) follow a GPU pipeline that way.  With the parameters ``format``
(a raw format of ``ops.yuv``), ``height`` and ``width``, ``images`` must be raw ``[B, frame_bytes]``
frames, and ``format``, ``height`` and ``width`` are emitted next to them.
"""
from __future__ import annotations

import numpy as np
import torch

from ...gpu.element import DeviceResult, FramePool, GpuPipelineElement, HostRing
from ...pipeline.stream import StreamEvent

__all__ = ["FrameDownload", "RgbToYuv"]


class RgbToYuv(GpuPipelineElement):
    lane_safe = True          # output buffers per lane, pool slots per frame

    def __init__(self, context):
        context.set_protocol("rgb_to_yuv:0")
        super().__init__(context)
        from ...ops import require_native
        from ...ops import yuv as Y
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.format = str(p("format", "nv12")).lower()
        self.standard = str(p("standard", "bt601")).lower()
        if self.format not in Y.FORMATS:
            raise ValueError(f"RgbToYuv: unknown format {self.format!r} (one of {sorted(Y.FORMATS)})")
        if self.standard not in Y.ENCODE_STANDARDS:
            raise ValueError(f"RgbToYuv: unknown standard {self.standard!r} (one of {sorted(Y.ENCODE_STANDARDS)})")
        self.pool_slots = int(p("pool", 0))
        self._out = {}
        self._pools = {}

    def _convert(self, rgb, out):
        from ...ops import yuv as Y
        return Y.rgb_to_yuv(rgb, self.format, self.standard, out=out)

    def process_frame(self, stream, images):
        from ...ops.yuv import frame_bytes
        if images.dim() != 4 or images.shape[3] != 3:
            raise ValueError(f"RgbToYuv: images [B, H, W, 3] required, got {tuple(images.shape)}")
        B, H, W = images.shape[:3]
        shape = (B, frame_bytes(self.format, H, W))       # yuyv with an odd width: ValueError
        if self.pool_slots > 0:
            pool = self._pools.get(shape)
            if pool is None:
                pool = self._pools[shape] = FramePool(self.pool_slots, shape[0] * shape[1], device=self.device)
            slot = pool.acquire(30.0)
            if slot >= 0:
                out = pool.view(slot, shape, torch.uint8)
                self.hold_for_frame(pool, slot)
                from ...parallel.hop import mark_frame_held
                # the output changes with the slot: a direct launch (a single kernel either way)
                return StreamEvent.OKAY, {"images": mark_frame_held(self._convert(images, out))}
        key = (B, H, W, self.lane)
        out = self._out.get(key)
        if out is None:
            out = self._out[key] = torch.empty(shape, dtype=torch.uint8, device=self.device)
        raw = self.run_maybe_captured(("rgb_yuv", B, H, W), lambda rgb: self._convert(rgb, out), images)
        return StreamEvent.OKAY, {"images": raw}


class _HeldFrame(np.ndarray):
    """A frame in a pinned host set: every view of it keeps ``hold`` (the set's DeviceResult)
    alive, and with it the set out of the ring's hands."""
    hold = None

    def __array_finalize__(self, obj):
        self.hold = getattr(obj, "hold", None)


class FrameDownload(GpuPipelineElement):
    lane_safe = True          # a pinned ring per (shape, lane)

    def __init__(self, context):
        context.set_protocol("frame_download:0")
        super().__init__(context)
        self.format = str(self.get_parameter("format", "rgb")[0]).lower()
        self.height = self.width = self.frame_bytes = None
        if self.format != "rgb":
            from ...ops.yuv import frame_bytes
            height, width = self.get_parameter("height", None)[0], self.get_parameter("width", None)[0]
            if height is None or width is None:
                raise ValueError(f"FrameDownload: format {self.format} needs height and width parameters")
            self.height, self.width = int(height), int(width)
            self.frame_bytes = frame_bytes(self.format, self.height, self.width)     # unknown format: ValueError
        self.ring_sets = max(2, int(self.get_parameter("ring", 4)[0]))
        self._rings = {}
        self.bytes_downloaded = 0

    def process_frame(self, stream, images):
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() < 1:
            raise ValueError("FrameDownload: images must be a uint8 tensor [B, ...]")
        if self.frame_bytes is not None and (images.dim() != 2 or images.shape[1] != self.frame_bytes):
            raise ValueError(f"FrameDownload: raw {self.format} frames of {self.height} x {self.width} are "
                             f"[B, {self.frame_bytes}], got images {tuple(images.shape)}")
        shape = tuple(images.shape)
        cuda = images.is_cuda
        key = (shape, self.lane)
        ring = self._rings.get(key)
        if ring is None:
            ring = self._rings[key] = HostRing(lambda: torch.empty(shape, dtype=torch.uint8, pin_memory=cuda),
                                               self.ring_sets)
        slot, host = ring.acquire()
        host.copy_(images, non_blocking=True)
        ev = None
        if cuda:
            ev = torch.cuda.Event()
            ev.record()
        hold = ring.bind(slot, DeviceResult({"images": host}, ev))
        hold.wait()                                       # this copy's event, nothing else on the device
        frames = []
        for frame in host.numpy():
            frame = frame.view(_HeldFrame)
            frame.hold = hold
            frames.append(frame)
        self.bytes_downloaded += images.numel()
        out = {"images": frames}
        if self.frame_bytes is not None:
            out.update(format=self.format, height=self.height, width=self.width)
        return StreamEvent.OKAY, out
