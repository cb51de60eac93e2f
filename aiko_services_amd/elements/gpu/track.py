"""Object identity across frames on the device: the tracker behind a video detector.

    "(SyntheticFrames YoloDetector DetectionTracker DetectionOverlay)"
        DetectionOverlay name_format: "#{i}" — every box labelled and coloured by its track

* ``DetectionTracker`` — the ``YoloDetector``'s ``detections`` ``[B, max_det, 6]`` / ``counts``
  ``[B]`` -> ``track_ids``, ``track_hits`` and ``labels``, int32 ``[B*rois]`` (slot ``b*rois + i`` =
  box ``i`` of frame ``b``, the layout of ``RoiCrop`` and of ``DetectionOverlay``'s ``labels``);
  ``detections`` and ``counts`` pass through.  Batch row ``b`` is camera ``b`` and successive
  pipeline frames are successive instants: the row's table of ``tracks`` slots stays in HBM and one
  launch of ``track_ops.hip`` (:func:`~aiko_services_amd.ops.track.track_detections`, which states
  the rules) advances it.  Nothing is copied to the host and nothing synchronises.
* ``TrackResults`` — the host sink: ``detections`` / ``counts`` / ``track_ids`` / ``track_hits``
  into pinned host memory without synchronising, emitted as one :class:`DeviceResult`.

Parameters of ``DetectionTracker``: ``rois`` (8 boxes considered per frame, at most 64), ``tracks``
(32 slots per row, at most 64), ``iou`` (0.3), ``max_age`` (30 frames without a match), ``min_score``
(0.0: the score a detection needs to start a track), ``class_aware`` (true), ``label_mod`` (1000:
``labels`` = id modulo this, the overlay's name table has that many entries).

Frame k reads the state frame k-1 wrote and writes its own, into set k % R of a ring of R =
max(2, lanes + 1) (state, outputs) sets, and waits for frame k-1's launch first (an event chain
across the lane streams), as ``AudioResample`` does: set k % R was last written by frame k-R, all
of whose work — the readers of its outputs further down the graph included — ran on frame k-1's
lane before frame k-1's launch, and last read as a state by frame k-R+1, whose launch the chain
orders before (or is) frame k-1's.  The state starts empty and is reset when ``B`` changes.
"""
from __future__ import annotations

import torch

from ...gpu.element import DeviceResult, GpuPipelineElement, HostRing
from ...pipeline.stream import StreamEvent

__all__ = ["DetectionTracker", "TrackResults"]


def _flag(value) -> bool:
    return str(value).lower() in ("true", "1", "yes")


class DetectionTracker(GpuPipelineElement):
    lane_safe = True          # state and output ring, ordered by an event chain

    def __init__(self, context):
        context.set_protocol("detection_tracker:0")
        super().__init__(context)
        from ...ops import require_native
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.k = int(p("rois", 8))
        self.tracks = int(p("tracks", 32))
        if not 1 <= self.k <= 64 or not 1 <= self.tracks <= 64:
            raise ValueError(f"DetectionTracker: 1 <= rois, tracks <= 64 required, got {self.k}, {self.tracks}")
        self.options = dict(iou=float(p("iou", 0.3)), max_age=int(p("max_age", 30)),
                            min_score=float(p("min_score", 0.0)), class_aware=_flag(p("class_aware", True)),
                            label_mod=int(p("label_mod", 1000)))
        self._ring = None
        self._cur = 0
        self._last = None

    def process_frame(self, stream, detections, counts):
        from ...ops import track as T
        if not isinstance(detections, torch.Tensor) or detections.dim() != 3 or detections.shape[1] < self.k:
            return StreamEvent.ERROR, {"diagnostic": f"DetectionTracker: detections [B, max_det >= rois = {self.k}, 6] "
                                                     f"required, got {tuple(getattr(detections, 'shape', ()))}"}
        B = detections.shape[0]
        lanes = getattr(self.pipeline, "_lanes_cfg", (1, None))[0] if self.pipeline is not None else 1
        R = max(2, lanes + 1)
        ring = self._ring
        if ring is None or len(ring) != R or ring[0][0].boxes.shape[0] != B:
            ring = self._ring = [(T.new_state(B, self.tracks, self.device),
                                  tuple(torch.empty(B * self.k, dtype=torch.int32, device=self.device)
                                        for _ in range(3))) for _ in range(R)]
            self._cur = 0
        state = ring[self._cur][0]
        self._cur = (self._cur + 1) % R
        state_out, (ids, hits, labels) = ring[self._cur]
        if self._last is not None:
            torch.cuda.current_stream(self.device).wait_event(self._last)
        T.track_detections(detections, counts, state, self.k, state_out=state_out, ids=ids, hits=hits,
                           labels=labels, **self.options)
        self._last = torch.cuda.Event()
        self._last.record()
        return StreamEvent.OKAY, {"track_ids": ids, "track_hits": hits, "labels": labels,
                                  "detections": detections, "counts": counts}


class TrackResults(GpuPipelineElement):
    """``detections`` fp32 ``[B, max_det, 6]``, ``counts`` int32 ``[B]``, ``track_ids`` and
    ``track_hits`` int32 ``[B*K]`` -> ``tracks``: a :class:`DeviceResult` of pinned host copies
    ``det`` / ``count`` / ``ids`` / ``hits`` and the event that completes them."""
    lane_safe = True          # pinned host ring per lane

    def __init__(self, context):
        context.set_protocol("track_results:0")
        super().__init__(context)
        self._rings = {}

    def process_frame(self, stream, detections, counts, track_ids, track_hits, t_submit=None):
        sources = (detections, counts, track_ids, track_hits)
        key = (tuple(detections.shape), tuple(track_ids.shape), self.lane)
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
        result = DeviceResult(dict(zip(("det", "count", "ids", "hits"), host)), ev,
                              t_submit=t_submit if isinstance(t_submit, (float, torch.Tensor)) else None)
        return StreamEvent.OKAY, {"tracks": ring.bind(slot, result)}
