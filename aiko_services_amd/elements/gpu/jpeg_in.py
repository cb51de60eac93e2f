"""Compressed frames into the pipeline on the device: baseline JPEG / Motion-JPEG.

    "(VideoReadFile JpegDecode YoloDetector DetectionOverlay JpegEncode JpegResults VideoWriteFile)"
        VideoReadFile raw: true on an MJPG .avi — MJPG in, MJPG out, no host codec in the graph

``JpegDecode`` — coded frames -> ``images`` device uint8 ``[B, H, W, 3]`` RGB (``output: rgb``, the default)
or the raw ``[B, frame_bytes]`` frames of the stream's sampling (``output: raw``: ``i420`` for 4:2:0,
``yuyv`` for 4:2:2, ``i444`` for 4:4:4), and ``status`` int32 ``[B]`` on the device, 0 for a frame that
decoded (the bits: :mod:`~aiko_services_amd.ops.jpeg_decode`, which states the whole rule).  The three
launches of ``jpeg_decode_ops.hip`` and, for RGB, ``yuv_to_rgb`` (``standard="jpeg"``) run inside one
``run_maybe_captured``; nothing synchronises with the device.

* ``input: host`` (default) — ``images`` is a list of B coded frames (bytes or 1-D uint8 arrays, as
  ``VideoReadFile`` with ``raw: true`` reads them from an MJPG ``.avi``).  The headers are parsed on the
  host (cached: an MJPG stream repeats them), the frames packed into a pinned ring and uploaded on the
  lane's stream; ``bytes_uploaded`` counts the coded bytes.  The format and size are the first batch's,
  or the ``height`` / ``width`` / ``subsampling`` parameters'; a frame of another format or size, and a
  stream the decoder does not take (``JpegUnsupported``: progressive, grayscale, ...), is an error
  that says why.
* ``input: device`` — ``images`` uint8 ``[B, cap]`` and ``nbytes`` int32 ``[B]`` as ``JpegEncode`` emits them,
  with that element's ``quality`` and ``subsampling`` and the ``height`` and ``width`` parameters: the
  header is known without a byte visiting the host.  An overflowed frame (``nbytes`` -1) has status 1.

Buffers are per (shape, lane).
"""
from __future__ import annotations

import torch

from ...gpu.element import DeviceResult, GpuPipelineElement, HostRing
from ...pipeline.stream import StreamEvent

__all__ = ["JpegDecode"]

_SUBSAMPLING = {"420": "i420", "422": "yuyv", "444": "i444", "i420": "i420", "yuyv": "yuyv", "i444": "i444",
                "4:2:0": "i420", "4:2:2": "yuyv", "4:4:4": "i444"}


class JpegDecode(GpuPipelineElement):
    lane_safe = True          # buffers per (shape, lane)

    def __init__(self, context):
        context.set_protocol("jpeg_decode:0")
        super().__init__(context)
        from ...ops import jpeg as J
        from ...ops import jpeg_decode as D
        from ...ops import require_native
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.input = str(p("input", "host")).lower()
        if self.input not in ("host", "device"):
            raise ValueError(f"JpegDecode: input host or device required, got {self.input!r}")
        self.output = str(p("output", "rgb")).lower()
        if self.output not in ("rgb", "raw"):
            raise ValueError(f"JpegDecode: output rgb or raw required, got {self.output!r}")
        sub, height, width = p("subsampling", None), p("height", None), p("width", None)
        if sub is not None and str(sub).lower() not in _SUBSAMPLING:
            raise ValueError(f"JpegDecode: subsampling 420, 422 or 444 required, got {sub!r}")
        self.format = None if sub is None else _SUBSAMPLING[str(sub).lower()]
        self.height = None if height is None else int(height)
        self.width = None if width is None else int(width)
        self.plan = None
        self._desc = {}
        if self.input == "device":
            if self.height is None or self.width is None:
                raise ValueError("JpegDecode: input device needs the height and width parameters")
            self.format = self.format or "i420"
            if self.format not in J.JPEG_FORMATS:
                raise ValueError("JpegDecode: input device takes what JpegEncode writes: subsampling 420 or 444")
            quality = p("quality", 90)
            quality = J._check_quality(int(quality) if isinstance(quality, str) and quality.strip().isdigit()
                                       else quality)
            self.plan = D.parse(J.header(self.format, self.height, self.width, quality))
        elif None not in (self.format, self.height, self.width):
            D.geometry(self.format, self.height, self.width)
        self._rings = {}
        self._events = {}
        self._buffers = {}
        self.bytes_uploaded = 0

    def _outputs(self, B, H, W, fmt, restart_interval):
        from ...ops import jpeg_decode as D
        from ...ops.yuv import frame_bytes
        key = ("out", B, H, W, fmt, restart_interval, self.lane)
        buffers = self._buffers.get(key)
        if buffers is None:
            dev = self.device
            buffers = self._buffers[key] = dict(
                raw=torch.empty(B, frame_bytes(fmt, H, W), dtype=torch.uint8, device=dev),
                status=torch.empty(B, dtype=torch.int32, device=dev),
                workspace=torch.empty(D.workspace_bytes(fmt, H, W, B, restart_interval), dtype=torch.uint8, device=dev),
                rgb=torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev) if self.output == "rgb" else None)
        return buffers

    def _decode(self, key, fmt, H, W, restart_interval, buffers, data, nbytes, desc):
        from ...ops import jpeg_decode as D
        from ...ops.yuv import yuv_to_rgb

        def decode(data, nbytes, desc):
            raw, status = D.jpeg_decode(data, nbytes, desc, H, W, fmt, restart_interval=restart_interval,
                                        raw=buffers["raw"], status=buffers["status"], workspace=buffers["workspace"])
            if self.output == "rgb":
                return yuv_to_rgb(raw, H, W, fmt, "jpeg", out=buffers["rgb"]), status
            return raw, status

        images, status = self.run_maybe_captured(key, decode, data, nbytes, desc)
        return StreamEvent.OKAY, {"images": images, "status": status}

    def process_frame(self, stream, images, nbytes=None):
        if self.input == "device":
            return self._from_device(images, nbytes)
        return self._from_host(images)

    def _from_device(self, images, nbytes):
        from ...ops import jpeg_decode as D
        ok = isinstance(images, torch.Tensor) and images.dtype == torch.uint8 and images.dim() == 2 and \
            images.device.type == "cuda" and images.is_contiguous() and isinstance(nbytes, torch.Tensor) and \
            nbytes.dtype == torch.int32 and tuple(nbytes.shape) == (images.shape[0],) and nbytes.device == images.device
        if not ok:
            return StreamEvent.ERROR, {"diagnostic": "JpegDecode: images uint8 [B, cap] and nbytes int32 [B] on the "
                                                     "device required (input: device)"}
        plan, (B, cap) = self.plan, images.shape
        desc = self._desc.get(self.lane)
        if desc is None:
            desc = self._desc[self.lane] = D.plan_bytes(plan)[None].to(self.device)
        buffers = self._outputs(B, plan.height, plan.width, plan.fmt, plan.restart_interval)
        return self._decode(("jpeg_decode", B, cap), plan.fmt, plan.height, plan.width, plan.restart_interval, buffers,
                            images, nbytes, desc)

    def _from_host(self, images):
        from ...ops import jpeg_decode as D
        from ...ops.yuv import frame_bytes
        if not isinstance(images, (list, tuple)) or not images:
            return StreamEvent.ERROR, {"diagnostic": "JpegDecode: images a list of coded frames required (input: "
                                                     f"host), got {type(images).__name__}"}
        B = len(images)
        try:
            first = D.parse(images[0])
        except ValueError as exc:
            return StreamEvent.ERROR, {"diagnostic": f"JpegDecode: frame 0 of the batch: {exc}"}
        want = (self.format or first.fmt, self.height or first.height, self.width or first.width)
        if (first.fmt, first.height, first.width) != want:
            return StreamEvent.ERROR, {"diagnostic": f"JpegDecode: a frame of {first.fmt} {first.height} x {first.width} "
                                                     f"in a stream of {want[0]} {want[1]} x {want[2]}"}
        self.format, self.height, self.width = fmt, H, W = want
        longest = max(len(f) for f in images)
        cap = max(frame_bytes(fmt, H, W) + 4096, longest + 4095) // 4096 * 4096
        key = (B, cap, self.lane)
        ring = self._rings.get(key)
        if ring is None:
            pin = self.device.type == "cuda"
            ring = self._rings[key] = HostRing(
                lambda: (torch.zeros(B, cap, dtype=torch.uint8, pin_memory=pin),
                         torch.zeros(B, dtype=torch.int32, pin_memory=pin),
                         torch.zeros(B, D.PLAN_BYTES, dtype=torch.uint8, pin_memory=pin)), 4)
            dev = self.device
            self._buffers[key] = (torch.empty(B, cap, dtype=torch.uint8, device=dev),
                                  torch.empty(B, dtype=torch.int32, device=dev),
                                  torch.empty(B, D.PLAN_BYTES, dtype=torch.uint8, device=dev))
        slot, host = ring.acquire()
        last = self._events.get((key, slot))
        if last is not None:
            last.synchronize()                              # the upload that last read this set is done
        try:
            D.pack(list(images), out=host)
        except ValueError as exc:                           # JpegUnsupported, or a frame of another size
            return StreamEvent.ERROR, {"diagnostic": f"JpegDecode: {exc}"}
        device = self._buffers[key]
        coded = int(host[1].sum())
        width = min(cap, (int(host[1].max()) + 255) // 256 * 256)
        device[0][:, :width].copy_(host[0][:, :width], non_blocking=True)
        device[1].copy_(host[1], non_blocking=True)
        device[2].copy_(host[2], non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self._events[(key, slot)] = event
        ring.bind(slot, DeviceResult({}, event))            # dropped at once: the event guards the set
        self.bytes_uploaded += coded
        self.share["bytes_uploaded"] = self.bytes_uploaded
        buffers = self._outputs(B, H, W, fmt, None)
        return self._decode(("jpeg_decode", B, cap), fmt, H, W, None, buffers, *device)
