"""Compressed frames out of the pipeline on the device: baseline JPEG / Motion-JPEG.

    "(SyntheticFrames YoloDetector DetectionOverlay JpegEncode JpegResults VideoWriteFile)"
        VideoWriteFile raw: true, format: jpeg — an MJPG .avi without a host encode

* ``JpegEncode`` — ``images`` device uint8 ``[B, H, W, 3]`` RGB (or raw ``[B, frame_bytes]`` planar
  frames) -> ``images`` uint8 ``[B, cap]``, one complete JFIF stream per row, and ``nbytes`` int32
  ``[B]``, its length (-1: the stream did not fit ``cap``).  For RGB it runs
  :func:`~aiko_services_amd.ops.yuv.rgb_to_yuv` (``standard="jpeg"``: full range, centre-sited chroma,
  which is JPEG's) into a buffer of its own and then the two launches of ``jpeg_ops.hip``
  (:func:`~aiko_services_amd.ops.jpeg.jpeg_encode`, which states the rule), all inside one
  ``run_maybe_captured``.  Nothing is copied to the host and nothing synchronises.
* ``JpegResults`` — the host sink: ``nbytes`` into pinned host memory, a wait for that copy's event
  only, then the first ``max(nbytes)`` columns of ``images``.  It emits ``images`` as a list of B
  byte arrays, views of the pinned set trimmed to their lengths, and ``format: "jpeg"``; an overflowed
  frame is an error that names the frame and ``cap``.

Parameters of ``JpegEncode``: ``quality`` (90, 1..100), ``subsampling`` (``420`` | ``444``), ``input``
(``rgb`` | ``i420`` | ``i444``; the raw inputs need ``height`` and ``width`` and fix the subsampling),
``cap`` (bytes per stream; by default the header plus the raw frame, which only noise at the highest
qualities exceeds).  Buffers are per (shape, lane), as ``RgbToYuv``'s with ``pool: 0``.
"""
from __future__ import annotations

import torch

from ...gpu.element import DeviceResult, GpuPipelineElement, HostRing
from ...pipeline.stream import StreamEvent
from .egress import _HeldFrame

__all__ = ["JpegEncode", "JpegResults"]

_SUBSAMPLING = {"420": "i420", "444": "i444", "i420": "i420", "i444": "i444", "4:2:0": "i420", "4:4:4": "i444"}


class JpegEncode(GpuPipelineElement):
    lane_safe = True          # buffers per (shape, lane)

    def __init__(self, context):
        context.set_protocol("jpeg_encode:0")
        super().__init__(context)
        from ...ops import require_native
        from ...ops import jpeg as J
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        quality = p("quality", 90)
        self.quality = J._check_quality(int(quality) if isinstance(quality, str) and quality.strip().isdigit()
                                        else quality)
        self.input = str(p("input", "rgb")).lower()
        if self.input not in ("rgb", "i420", "i444"):
            raise ValueError(f"JpegEncode: input one of rgb, i420, i444 required, got {self.input!r}")
        sub = str(p("subsampling", "420" if self.input == "rgb" else self.input)).lower()
        if sub not in _SUBSAMPLING:
            raise ValueError(f"JpegEncode: subsampling 420 or 444 required, got {sub!r}")
        self.format = _SUBSAMPLING[sub]
        self.height = self.width = None
        if self.input != "rgb":
            if self.format != self.input:
                raise ValueError(f"JpegEncode: input {self.input} is coded as it is: subsampling {sub} does not apply")
            height, width = p("height", None), p("width", None)
            if height is None or width is None:
                raise ValueError(f"JpegEncode: input {self.input} needs the height and width parameters")
            self.height, self.width = int(height), int(width)
            J.geometry(self.format, self.height, self.width)
        cap = p("cap", None)
        self.cap = None if cap is None else int(cap)
        if self.cap is not None and self.cap < 1:
            raise ValueError(f"JpegEncode: cap >= 1 required, got {self.cap}")
        self._buffers = {}

    def process_frame(self, stream, images):
        from ...ops import jpeg as J
        from ...ops.yuv import frame_bytes, rgb_to_yuv
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.device.type != "cuda" or \
                not images.is_contiguous():
            return StreamEvent.ERROR, {"diagnostic": "JpegEncode: images uint8 contiguous on the device required, got "
                                                     f"{tuple(getattr(images, 'shape', ()))} "
                                                     f"{getattr(images, 'dtype', type(images).__name__)}"}
        fmt, quality = self.format, self.quality
        if self.input == "rgb":
            if images.dim() != 4 or images.shape[3] != 3:
                return StreamEvent.ERROR, {"diagnostic": f"JpegEncode: images [B, H, W, 3] required, got "
                                                         f"{tuple(images.shape)}"}
            B, H, W = images.shape[:3]
        else:
            B, H, W = images.shape[0], self.height, self.width
            if images.dim() != 2 or images.shape[1] != frame_bytes(fmt, H, W):
                return StreamEvent.ERROR, {"diagnostic": f"JpegEncode: raw {fmt} frames of {H} x {W} are [B, "
                                                         f"{frame_bytes(fmt, H, W)}], got {tuple(images.shape)}"}
        try:
            my = J.geometry(fmt, H, W)[3]
        except ValueError as exc:
            return StreamEvent.ERROR, {"diagnostic": f"JpegEncode: {exc}"}
        key = (B, H, W, self.lane)
        buffers = self._buffers.get(key)
        if buffers is None:
            dcap, seg_cap = J.capacities(fmt, H, W)
            dev = self.device
            u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)  # noqa: E731
            buffers = self._buffers[key] = dict(
                raw=u8(B, frame_bytes(fmt, H, W)) if self.input == "rgb" else None,
                stream=u8(B, self.cap or dcap), nbytes=torch.empty(B, dtype=torch.int32, device=dev),
                workspace=u8(B * my * (4 + seg_cap)))
            J.device_tables(fmt, H, W, quality, dev)       # uploaded here, not inside a capture

        def encode(x):
            raw = rgb_to_yuv(x, fmt, "jpeg", out=buffers["raw"]) if self.input == "rgb" else x
            return J.jpeg_encode(raw, H, W, fmt, quality, stream=buffers["stream"], nbytes=buffers["nbytes"],
                                 workspace=buffers["workspace"])

        out, nbytes = self.run_maybe_captured(("jpeg", B, H, W), encode, images)
        return StreamEvent.OKAY, {"images": out, "nbytes": nbytes}


class JpegResults(GpuPipelineElement):
    """``images`` uint8 ``[B, cap]`` and ``nbytes`` int32 ``[B]`` -> ``images``: a list of B uint8 arrays
    in pinned host memory, each one JPEG file; ``nbytes``: their lengths; ``format``: ``"jpeg"``."""
    lane_safe = True          # pinned host ring per (shape, lane)

    def __init__(self, context):
        context.set_protocol("jpeg_results:0")
        super().__init__(context)
        self._rings = {}
        self.bytes_downloaded = 0

    def process_frame(self, stream, images, nbytes):
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 2 or \
                not isinstance(nbytes, torch.Tensor) or nbytes.dtype != torch.int32 or \
                tuple(nbytes.shape) != (images.shape[0],):
            return StreamEvent.ERROR, {"diagnostic": "JpegResults: images uint8 [B, cap] and nbytes int32 [B] required"}
        B, cap = images.shape
        cuda = images.is_cuda
        key = (B, cap, self.lane)
        ring = self._rings.get(key)
        if ring is None:
            ring = self._rings[key] = HostRing(
                lambda: (torch.empty(B, cap, dtype=torch.uint8, pin_memory=cuda),
                         torch.empty(B, dtype=torch.int32, pin_memory=cuda)), 4)
        slot, (host, lengths) = ring.acquire()
        lengths.copy_(nbytes, non_blocking=True)
        if cuda:
            ev = torch.cuda.Event()
            ev.record()
            ev.synchronize()                                # the lengths' copy, nothing else on the device
        counts = lengths.tolist()
        longest = max(counts)
        ev = None
        if longest > 0:
            host[:, :longest].copy_(images[:, :longest], non_blocking=True)
        if cuda:
            ev = torch.cuda.Event()
            ev.record()
        hold = ring.bind(slot, DeviceResult({"images": host, "nbytes": lengths}, ev))
        hold.wait()
        for b, n in enumerate(counts):
            if n < 0:
                return StreamEvent.ERROR, {"diagnostic": f"JpegResults: frame {b} of the batch did not fit cap = {cap} "
                                                         "bytes (or one of its restart segments its seg_cap): raise "
                                                         "JpegEncode's cap or lower its quality"}
        frames = []
        rows = host.numpy()
        for b, n in enumerate(counts):
            frame = rows[b, :n].view(_HeldFrame)
            frame.hold = hold
            frames.append(frame)
        self.bytes_downloaded += B * longest
        return StreamEvent.OKAY, {"images": frames, "nbytes": counts, "format": "jpeg"}
