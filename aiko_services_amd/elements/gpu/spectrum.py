"""Spectrum analysis on the device: the host chain ``PE_FFT -> PE_AudioFilter -> PE_AudioResampler ->
PE_GraphXY`` of ``elements/media/audio_io.py`` for every stream of a batch, with no host round trip.

    "(AudioChunks AudioResample AudioSpectrum SpectrumResults)"
        with ``graph: true`` the ``images`` go on to DetectionOverlay, RgbToYuv, JpegEncode or FrameDownload

* ``AudioSpectrum`` — ``audio`` fp32 ``[B, n]`` on the device (what ``AudioChunks`` and ``AudioResample``
  emit) -> ``amplitudes`` fp32 ``[B, K]`` (``K = n_fft/2 + 1``; a sine of amplitude ``A`` at a bin centre
  reads ``A``), ``band_amplitudes`` fp32 ``[B, band_count]`` (``PE_AudioResampler``'s sums),
  ``peak_bins`` int32 / ``peak_amplitudes`` fp32 ``[B, samples_maximum]`` and ``peak_counts`` int32
  ``[B]`` (``PE_AudioFilter``'s loudest points, -1 / 0 past the count), ``power`` fp32 ``[B, F, K]``
  (the spectrogram) and, with ``graph: true``, ``images`` uint8 ``[B, height, width, 3]``
  (``PE_GraphXY``'s scatter graph); ``audio`` passes through.  The two or three launches of
  ``spectrum_ops.hip`` (:func:`~aiko_services_amd.ops.spectrum.spectrum`, which states the rule).
  Nothing is copied to the host and nothing synchronises.  Stateless, a chunk is analysed on its own:
  one set of buffers per (shape, lane).
* ``SpectrumResults`` — the host sink: all but ``power`` and ``images`` into pinned host memory without
  synchronising, emitted as one :class:`DeviceResult`; :func:`to_host_spectrum` turns stream ``b`` of
  its result into the ``amplitudes`` / ``frequencies`` that ``PE_AudioFilter`` emits, so the host
  ``PE_AudioResampler`` (LED publishing) and ``PE_GraphXY`` work behind it unchanged.

Parameters of ``AudioSpectrum`` (scalars): ``sample_rate`` (16000), ``n_fft`` (1024; 256 .. 8192),
``hop`` (``n_fft / 2``), ``window`` (``hann``; ``hamming``, ``blackman``, ``rect``), ``band_count`` (8, at
most 64), ``frequency_band_maximum`` (8000), the host elements' ``amplitude_minimum`` (0.1),
``amplitude_maximum`` (12), ``frequency_minimum`` (10), ``frequency_maximum`` (9000) and
``samples_maximum`` (100, at most 128), ``local`` (false: with true a point must be a local maximum,
"the tones" instead of "the 100 loudest bins"), ``graph`` (false), ``width`` (640), ``height`` (480).
The graph's axes end at ``frequency_maximum`` and ``amplitude_maximum``, as ``PE_GraphXY``'s.
"""
from __future__ import annotations

import numpy as np
import torch

from ...gpu.element import DeviceResult, GpuPipelineElement, HostRing
from ...pipeline.stream import StreamEvent

__all__ = ["AudioSpectrum", "SpectrumResults", "to_host_spectrum"]


def _flag(v) -> bool:
    return v.strip().lower() in ("1", "true", "yes", "on") if isinstance(v, str) else bool(v)


class AudioSpectrum(GpuPipelineElement):
    lane_safe = True          # output buffers per lane

    def __init__(self, context):
        context.set_protocol("audio_spectrum:0")
        super().__init__(context)
        from ...ops import require_native
        from ...ops.spectrum import check_graph, check_parameters
        require_native()
        p = lambda name, d: self.get_parameter(name, d)[0]  # noqa: E731
        n_fft = int(p("n_fft", 1024))
        hop = p("hop", None)
        self.options = dict(sample_rate=float(p("sample_rate", 16000)), n_fft=n_fft,
                            hop=int(hop) if hop is not None else n_fft // 2, window=str(p("window", "hann")),
                            band_count=int(p("band_count", 8)),
                            frequency_band_maximum=float(p("frequency_band_maximum", 8000)),
                            amplitude_minimum=float(p("amplitude_minimum", 0.1)),
                            amplitude_maximum=float(p("amplitude_maximum", 12)),
                            frequency_minimum=float(p("frequency_minimum", 10)),
                            frequency_maximum=float(p("frequency_maximum", 9000)),
                            max_peaks=int(p("samples_maximum", 100)), local=_flag(p("local", False)))
        check_parameters(**self.options)
        self.graph = None
        if _flag(p("graph", False)):
            self.graph = dict(height=int(p("height", 480)), width=int(p("width", 640)))
            check_graph(self.graph["height"], self.graph["width"], self.options["frequency_maximum"],
                        self.options["amplitude_maximum"], (0, 255, 0))
        self._out = {}

    def process_frame(self, stream, audio):
        from ...ops import spectrum as S
        if not isinstance(audio, torch.Tensor) or audio.dim() != 2 or audio.dtype != torch.float32 or \
                audio.device.type != "cuda" or not audio.is_contiguous():
            return StreamEvent.ERROR, {"diagnostic": "AudioSpectrum: audio fp32 [B, n] contiguous on the device "
                                                     f"required, got {tuple(getattr(audio, 'shape', ()))} "
                                                     f"{getattr(audio, 'dtype', type(audio).__name__)}"}
        B, n = audio.shape
        o = self.options
        F = S.frame_count(n, o["n_fft"], o["hop"]) if n >= 1 else 0
        if B < 1 or not 1 <= F <= S.MAX_FRAMES:
            return StreamEvent.ERROR, {"diagnostic": f"AudioSpectrum: a chunk of {n} samples is {F} frames of "
                                                     f"{o['n_fft']} at hop {o['hop']}, not 1..{S.MAX_FRAMES}"}
        key = (B, n, self.lane)
        out = self._out.get(key)
        if out is None:
            dev, K, P = self.device, o["n_fft"] // 2 + 1, o["max_peaks"]
            f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
            out = self._out[key] = dict(amplitudes=f32(B, K), band_amplitudes=f32(B, o["band_count"]),
                                        peak_bins=torch.empty(B, P, dtype=torch.int32, device=dev),
                                        peak_amplitudes=f32(B, P),
                                        peak_counts=torch.empty(B, dtype=torch.int32, device=dev), power=f32(B, F, K))
            if self.graph is not None:
                out["image"] = torch.empty(B, self.graph["height"], self.graph["width"], 3, dtype=torch.uint8,
                                           device=dev)
        S.spectrum(audio, **o, graph=self.graph, **out)
        swag = {k: v for k, v in out.items() if k != "image"}
        if self.graph is not None:
            swag["images"] = out["image"]
        swag["audio"] = audio
        return StreamEvent.OKAY, swag


def to_host_spectrum(result, b: int, sample_rate=16000, n_fft: int = 1024) -> dict:
    """Stream ``b``'s peaks of a ``SpectrumResults`` result (a :class:`DeviceResult`, waited for here, or
    its dict) as the host ``PE_AudioFilter`` emits them: ``{"amplitudes": fp64 [count], "frequencies":
    fp64 [count]}``, loudest first."""
    from ...ops.spectrum import frequencies
    host = result.wait() if hasattr(result, "wait") else result
    n = int(host["peak_counts"][b])
    bins = host["peak_bins"][b, :n].numpy()
    return {"amplitudes": host["peak_amplitudes"][b, :n].numpy().astype(np.float64),
            "frequencies": frequencies(n_fft, sample_rate)[bins]}


class SpectrumResults(GpuPipelineElement):
    """``amplitudes`` fp32 ``[B, K]``, ``band_amplitudes`` fp32 ``[B, band_count]``, ``peak_bins`` int32 and
    ``peak_amplitudes`` fp32 ``[B, samples_maximum]`` and ``peak_counts`` int32 ``[B]`` -> ``spectrum``: a
    :class:`DeviceResult` of pinned host copies under the same names and the event that completes
    them (:func:`to_host_spectrum` makes the host ``PE_AudioFilter``'s outputs of it)."""
    lane_safe = True          # pinned host ring per lane
    NAMES = ("amplitudes", "band_amplitudes", "peak_bins", "peak_amplitudes", "peak_counts")

    def __init__(self, context):
        context.set_protocol("spectrum_results:0")
        super().__init__(context)
        self._rings = {}

    def process_frame(self, stream, amplitudes, band_amplitudes, peak_bins, peak_amplitudes, peak_counts,
                      t_submit=None):
        sources = (amplitudes, band_amplitudes, peak_bins, peak_amplitudes, peak_counts)
        key = (tuple(amplitudes.shape), tuple(band_amplitudes.shape), tuple(peak_bins.shape), self.lane)
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
        result = DeviceResult(dict(zip(self.NAMES, host)), ev,
                              t_submit=t_submit if isinstance(t_submit, (float, torch.Tensor)) else None)
        return StreamEvent.OKAY, {"spectrum": ring.bind(slot, result)}
