"""Raw PCM audio into the speech pipeline on the device.

    "(AudioReadFile AudioChunks AudioResample AudioWindow WhisperEncoder FeatureSink)"
        AudioReadFile raw: true, AudioChunks format: pcm16 — a 48 kHz stereo WAV file as it is stored

``AudioResample`` — ``audio`` device int16 or fp32 ``[B, n_in*C]`` or ``[B, n_in, C]`` (interleaved
PCM at ``sample_rate_in``, as ``AudioChunks`` with ``format: pcm16`` emits it) -> ``audio`` fp32
``[B, n_out]`` mono at ``sample_rate_out``, which ``AudioWindow`` takes: one launch of
``resample_ops.hip`` (:func:`~aiko_services_amd.ops.audio.resample`), device to device, no
synchronisation.  The filter is a Kaiser-windowed sinc low-pass below the lower Nyquist frequency
(:func:`~aiko_services_amd.ops.audio.resample_filter`); the output lags the input by
``resample_delay`` seconds, published in the element's share.

Parameters: ``sample_rate_in`` (48000), ``sample_rate_out`` (16000), ``channels`` (1), ``zeros``
(16), ``beta`` (9.0), ``rolloff`` (0.9).  A chunk must hold a multiple of ``M`` samples per channel,
``M = sample_rate_in / gcd(sample_rate_in, sample_rate_out)`` (3 for 48 kHz, 441 for 44.1 kHz), so
that every chunk starts at filter phase 0; any other length ends the frame with an ``ERROR``.

The last ``T-1`` mono samples of each stream stay on the device between frames.  Frame k reads the
history frame k-1 wrote and writes its own, into slot k % R of a ring of R = lanes + 1 (history,
output) pairs, and waits for frame k-1's launch first (an event chain across the lane streams), as
``AudioWindow`` does: slot k % R was last used by frame k-R, all of whose work ran on frame k-1's
lane before frame k-1's launch.  The history starts as zeros and is reset when ``B`` changes.
"""
from __future__ import annotations

import torch

from ...gpu.element import GpuPipelineElement
from ...pipeline.stream import StreamEvent

__all__ = ["AudioResample"]


class AudioResample(GpuPipelineElement):
    lane_safe = True          # history and output ring, ordered by an event chain

    def __init__(self, context):
        context.set_protocol("audio_resample_gpu:0")
        super().__init__(context)
        from ...ops import audio as A
        from ...ops import require_native
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        self.rate_in, self.rate_out = int(p("sample_rate_in", 48000)), int(p("sample_rate_out", 16000))
        self.channels = int(p("channels", 1))
        if not 1 <= self.channels <= 8:
            raise ValueError(f"AudioResample: 1 <= channels <= 8 required, got {self.channels}")
        design = (self.rate_in, self.rate_out, int(p("zeros", 16)), float(p("beta", 9.0)), float(p("rolloff", 0.9)))
        filt, self.L, self.M = A.resample_filter(*design)           # a refused ratio: ValueError
        self.filt = filt.to(self.device)
        self.taps = filt.shape[1]
        self.share["resample_delay"] = A.resample_delay(*design)
        self._ring = None
        self._cur = 0
        self._last = None

    def process_frame(self, stream, audio):
        from ...ops import audio as A
        C = self.channels
        if not isinstance(audio, torch.Tensor) or audio.device.type != "cuda" or \
                audio.dtype not in (torch.int16, torch.float32):
            return StreamEvent.ERROR, {"diagnostic": "AudioResample: audio must be a device int16 or fp32 tensor"}
        if audio.dim() == 2 and audio.shape[1] % C == 0:
            pcm = audio.contiguous().view(audio.shape[0], audio.shape[1] // C, C)
        elif audio.dim() == 3 and audio.shape[2] == C:
            pcm = audio.contiguous()
        else:
            return StreamEvent.ERROR, {"diagnostic": f"AudioResample: audio [B, n*{C}] or [B, n, {C}] required, "
                                                     f"got {tuple(audio.shape)}"}
        B, n_in, _ = pcm.shape
        if n_in < 1 or (n_in * self.L) % self.M:
            return StreamEvent.ERROR, {"diagnostic": f"AudioResample: a chunk of {n_in} samples per channel is not a "
                                                     f"multiple of {self.M} ({self.rate_in} -> {self.rate_out} Hz)"}
        n_out = n_in * self.L // self.M
        lanes = getattr(self.pipeline, "_lanes_cfg", (1, None))[0] if self.pipeline is not None else 1
        R = max(2, lanes + 1)
        ring = self._ring
        if ring is None or len(ring) != R or ring[0][0].shape[0] != B or ring[0][1].shape[1] != n_out:
            carry = None
            if ring is not None and ring[0][0].shape[0] == B:       # the same streams, another chunk length
                carry = ring[self._cur][0]
            ring = self._ring = [(torch.zeros(B, self.taps - 1, dtype=torch.float32, device=self.device),
                                  torch.empty(B, n_out, dtype=torch.float32, device=self.device)) for _ in range(R)]
            self._cur = 0
            if carry is not None:
                if self._last is not None:
                    torch.cuda.current_stream(self.device).wait_event(self._last)
                ring[0][0].copy_(carry)
        hist = ring[self._cur][0]
        self._cur = (self._cur + 1) % R
        hist_out, out = ring[self._cur]
        if self._last is not None:
            torch.cuda.current_stream(self.device).wait_event(self._last)
        A.resample(pcm, hist, self.filt, self.L, self.M, out=out, hist_out=hist_out)
        self._last = torch.cuda.Event()
        self._last.record()
        return StreamEvent.OKAY, {"audio": out}
