"""Voice activity on the device: the cheap question before the expensive one.  Did anybody speak in
the last ``window`` seconds of this stream?  If not, the decoder has nothing to do.

    "(AudioChunks AudioResample VoiceActivity AudioWindow WhisperEncoder WhisperTranscribe)"
        WhisperTranscribe takes ``silent``: a silent stream's tokens are the prompt and end-of-text

* ``VoiceActivity`` — ``audio`` fp32 ``[B, n]`` at 16 kHz (what ``AudioChunks`` and ``AudioResample``
  emit; ``n`` whole frames of ``frame`` samples, at most 4096 of them) -> ``voice_mask`` uint8 ``[B,
  F]`` (1 where a frame is speech), ``voice_segments`` int32 ``[B, max_seg, 2]`` / ``voice_counts``
  int32 ``[B]`` (the runs of the mask as ``(first frame, one past the last)``), ``voice_speech`` int32
  ``[B]`` (speech frames in the chunk) and ``silent`` int32 ``[B]`` (1: no speech frame for ``window``
  seconds); ``audio`` passes through.  Batch row ``b`` is stream ``b`` and successive pipeline frames
  are successive chunks: the row's noise floor and counters stay in HBM and the two launches of
  ``vad_ops.hip`` (:func:`~aiko_services_amd.ops.vad.voice_activity`, which states the rule) advance
  them.  Nothing is copied to the host and nothing synchronises.
* ``VoiceResults`` — the host sink: ``voice_mask`` / ``voice_segments`` / ``voice_counts`` /
  ``voice_speech`` / ``silent`` into pinned host memory without synchronising, emitted as one
  :class:`DeviceResult`.

Parameters of ``VoiceActivity`` (scalars): those of the rule with its defaults — ``frame`` (320
samples: 20 ms; 160, 320 or 480), ``threshold`` (48 level units: 9 dB over the noise floor),
``min_level`` (0), ``up_shift`` (6), ``speech_shift`` (10), ``down_shift`` (1), ``warmup`` (10 frames),
``attack`` (3 frames), ``hang`` (15 frames), ``max_zc`` (479: off), ``max_seg`` (16 rows per chunk, at
most 64) — except ``window``, which is given in seconds (30.0: ``AudioWindow``'s default, what the
encoder sees).

Chunk k reads the state chunk k-1 wrote and writes its own, into set k % R of a ring of R =
max(2, lanes + 1) (state, outputs) sets, and waits for chunk k-1's launches first (an event chain
across the lane streams): ``MotionDetector``'s scheme, after ``DetectionTracker``'s, which argues why
a set is free when it is written again.  The state starts empty and is reset when ``B`` changes; a
change of the chunk length alone carries it over.
"""
from __future__ import annotations

import torch

from ...gpu.element import DeviceResult, GpuPipelineElement, HostRing
from ...pipeline.stream import StreamEvent

__all__ = ["VoiceActivity", "VoiceResults"]

RATE = 16000


class VoiceActivity(GpuPipelineElement):
    lane_safe = True          # state and output ring, ordered by an event chain

    def __init__(self, context):
        context.set_protocol("voice_activity:0")
        super().__init__(context)
        from ...ops import require_native
        from ...ops.vad import DEFAULTS, check_parameters
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.options = {name: int(p(name, d)) for name, d in DEFAULTS.items() if name != "window"}
        seconds = float(p("window", 30.0))
        self.options["window"] = max(1, round(seconds * RATE / self.options["frame"])) if seconds > 0 else 0
        check_parameters(**self.options)
        self._ring = None
        self._cur = 0
        self._last = None

    def process_frame(self, stream, audio):
        from ...ops import vad as V
        frame, max_seg = self.options["frame"], self.options["max_seg"]
        if not isinstance(audio, torch.Tensor) or audio.dim() != 2 or audio.dtype != torch.float32 or \
                audio.device.type != "cuda" or not audio.is_contiguous():
            return StreamEvent.ERROR, {"diagnostic": "VoiceActivity: audio fp32 [B, n] contiguous on the device "
                                                     f"required, got {tuple(getattr(audio, 'shape', ()))} "
                                                     f"{getattr(audio, 'dtype', type(audio).__name__)}"}
        B, n = audio.shape
        F = n // frame
        if B < 1 or n % frame or not 1 <= F <= V.MAX_FRAMES:
            return StreamEvent.ERROR, {"diagnostic": f"VoiceActivity: a chunk of {n} samples is not 1..{V.MAX_FRAMES} "
                                                     f"whole frames of {frame}"}
        lanes = getattr(self.pipeline, "_lanes_cfg", (1, None))[0] if self.pipeline is not None else 1
        R = max(2, lanes + 1)
        ring = self._ring
        if ring is None or len(ring) != R or ring[0][1][0].shape != (B, F):
            dev = self.device
            carry = None
            if ring is not None and ring[0][0].v.shape[0] == B:     # the same streams, another chunk length
                carry = ring[self._cur][0]
            i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)  # noqa: E731
            ring = self._ring = [(V.new_state(B, dev),
                                  (torch.empty(B, F, dtype=torch.uint8, device=dev), i32(B, max_seg, 2), i32(B), i32(B),
                                   i32(B), i32(B, F), i32(B, F))) for _ in range(R)]
            self._cur = 0
            if carry is not None:
                if self._last is not None:
                    torch.cuda.current_stream(self.device).wait_event(self._last)
                ring[0][0].v.copy_(carry.v)
            else:
                self._last = None
        state = ring[self._cur][0]
        self._cur = (self._cur + 1) % R
        state_out, (mask, seg, count, speech, silent, level, zc) = ring[self._cur]
        if self._last is not None:
            torch.cuda.current_stream(self.device).wait_event(self._last)
        V.voice_activity(audio, state, state_out=state_out, mask=mask, seg=seg, count=count, speech=speech,
                         silent=silent, level=level, zc=zc, **self.options)
        self._last = torch.cuda.Event()
        self._last.record()
        return StreamEvent.OKAY, {"voice_mask": mask, "voice_segments": seg, "voice_counts": count,
                                  "voice_speech": speech, "silent": silent, "audio": audio}


class VoiceResults(GpuPipelineElement):
    """``voice_mask`` uint8 ``[B, F]``, ``voice_segments`` int32 ``[B, max_seg, 2]``, ``voice_counts``,
    ``voice_speech`` and ``silent`` int32 ``[B]`` -> ``voice``: a :class:`DeviceResult` of pinned host
    copies ``mask`` / ``seg`` / ``count`` / ``speech`` / ``silent`` and the event that completes them."""
    lane_safe = True          # pinned host ring per lane

    def __init__(self, context):
        context.set_protocol("voice_results:0")
        super().__init__(context)
        self._rings = {}

    def process_frame(self, stream, voice_mask, voice_segments, voice_counts, voice_speech, silent, t_submit=None):
        sources = (voice_mask, voice_segments, voice_counts, voice_speech, silent)
        key = (tuple(voice_mask.shape), tuple(voice_segments.shape), self.lane)
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
        result = DeviceResult(dict(zip(("mask", "seg", "count", "speech", "silent"), host)), ev,
                              t_submit=t_submit if isinstance(t_submit, (float, torch.Tensor)) else None)
        return StreamEvent.OKAY, {"voice": ring.bind(slot, result)}
