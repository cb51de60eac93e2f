"""Spectrum analysis (``csrc/kernels/spectrum_ops.hip``): what is in this chunk, and how loud?  Batch
row ``b`` is one mono stream.  Out come the amplitude spectrum, its ``band_count`` bands (the host
``PE_AudioResampler``), its loudest points (the host ``PE_AudioFilter``), the frame powers (the
spectrogram) and, on request, the scatter graph of the points (the host ``PE_GraphXY``) as an image.
Two or three launches, no host copy, no synchronisation, hipGraph-capturable.  Stateless: a chunk is
analysed on its own, as the host ``PE_FFT`` does.

The rule, per row.  Every fp32 operation written below is rounded once (no fused multiply-add),
every fp64 operation likewise, so :func:`~aiko_services_amd.ops.reference.spectrum_ref` (numpy,
the same operations element-wise) equals the kernels bit for bit in every output.

``audio`` is fp32 ``[B, n]``, contiguous, ``n >= 1``.  ``n_fft`` is one of 256 .. 8192 (8192: a 0.1 s
chunk at 48 kHz, 4800 samples, is one zero-padded frame), ``K = n_fft/2 + 1``, ``hop`` in ``1..n_fft``
[``n_fft/2``].  The host tables are made once per parameter set (:func:`tables`), cached, and passed
to the kernels as tensors; the reference reads the same arrays:

* :func:`window` fp32 ``[n_fft]``: ``hann``, ``hamming``, ``blackman`` or ``rect`` in the periodic form,
  computed in fp64, multiplied by ``2 / sum(w)``, then rounded.  A sine of amplitude ``A`` at a bin
  centre then reads ``A``.  DC and the Nyquist bin have no mirror image to share their energy with
  and read double: a constant ``c`` reads ``2c`` at bin 0.
* :func:`twiddle` fp32 ``[n_fft/2, 2]`` = ``(fp32(cos(2 pi j / n_fft)), fp32(-sin(2 pi j / n_fft)))``.
* :func:`frequencies` fp64 ``[K]`` = ``np.fft.rfftfreq(n_fft, 1 / rate)``.

1. **Sample.**  NaN and +-inf read as 0, then clamp to ``[-32768, 32767]``: PCM given unnormalised is
   in range and nothing downstream can overflow.
2. **Frames.**  ``F = 1`` if ``n < n_fft`` else ``1 + (n - n_fft) // hop``, at most 4096.  Frame ``f`` is
   samples ``f*hop .. f*hop + n_fft - 1``; samples at or past ``n`` read 0 (only when ``n < n_fft``);
   samples past the last whole frame are not read.  ``v[i] = x[i] * w[i]``.
3. **Transform.**  A complex radix-2 decimation-in-time FFT of ``(v, 0)``: ``z[i] = v[bitrev(i)]``;
   for stage ``s = 1 .. log2 n_fft``, ``m = 2^s``, ``h = m/2``, every block of ``m`` and ``j < h``: ``a =
   z[j]``, ``b = z[j+h]``, ``(c, d) = twiddle[j * n_fft/m]``, ``t.re = b.re*c - b.im*d``, ``t.im = b.re*d +
   b.im*c``, ``z[j] = a + t``, ``z[j+h] = a - t``.
4. **Power.**  ``power[b, f, k] = re*re + im*im`` for ``k < K``: fp32 ``[B, F, K]``.
5. **Amplitude.**  ``acc = ((p[0] + p[1]) + ...)`` over the frames in order; ``amplitudes[b, k] =
   sqrt(acc * inv_F)``, ``inv_F = fp32(1 / F)``, the correctly rounded fp32 square root.
6. **Bands.**  ``band_count`` in ``1..64``, ``frequency_band_maximum > 0``.  ``edges = linspace(0, f_max,
   bands + 1)``, ``band_start = searchsorted(frequencies, edges, "left")`` int32 ``[bands + 1]``: bin
   ``k`` is in band ``j`` iff ``edges[j] <= f_k < edges[j+1]``.  ``band_amplitudes[b, j]`` is the
   sequential fp32 sum of the band's amplitudes in ascending ``k``; an empty band is 0.
7. **Peaks.**  ``max_peaks`` in ``1..128``.  A bin is kept iff ``lo <= a <= hi`` and ``k_lo <= k <=
   k_hi``: ``lo`` the smallest fp32 ``>= amplitude_minimum``, ``hi`` the largest fp32 ``<=
   amplitude_maximum`` (the fp32 comparison then equals the host element's comparison of the fp32
   value in fp64), ``k_lo = searchsorted(frequencies, frequency_minimum, "left")``, ``k_hi =
   searchsorted(frequencies, frequency_maximum, "right") - 1``.  With ``local`` a bin must also be a
   local maximum, ``a[k] > a[k-1]`` and ``a[k] >= a[k+1]``, a missing neighbour passing: "the 100
   loudest bins, all around one tone" become "the tones".  Of the kept bins the ``max_peaks`` largest
   by amplitude, ties to the lower bin: descending order of the key ``(bits(a) << 32) | (0xFFFFFFFF -
   k)``.  ``peak_bins`` int32 ``[B, max_peaks]`` (-1 past the count), ``peak_amplitudes`` fp32 (0 past
   the count), ``peak_counts`` int32 ``[B]``.
8. **Graph** (:func:`spectrum_graph`).  uint8 ``[B, H, W, 3]``, ``16 <= H, W <= 4096``, ``x_max, y_max >
   0``.  Zeros; row ``H-1`` and column 0 are 128.  For each peak ``i < count``: ``px =
   bin_px[peak_bin]``, ``bin_px[k] = clip(int(f_k / x_max * (W-1)), 0, W-1)`` int32 ``[K]`` from the
   host; ``py = clip(trunc((1.0 - (double)a / y_max) * (H-1)), 0, H-1)`` in fp64; the nine pixels
   ``(clip(py+dy), clip(px+dx))`` take ``color``.

Every element of every output is written.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np
import torch

__all__ = ["DEFAULTS", "MAX_FRAMES", "N_FFTS", "WINDOWS", "SpectrumOut", "Tables", "bin_pixels", "check_parameters",
           "frame_count", "frequencies", "spectrum", "spectrum_graph", "spectrum_uses_vector", "tables", "twiddle",
           "window"]

N_FFTS = (256, 512, 1024, 2048, 4096, 8192)
WINDOWS = ("hann", "hamming", "blackman", "rect")
MAX_FRAMES = 4096              # frames per call and stream (SP_MAX_F)
MAX_BANDS = 64
MAX_PEAKS = 128
DEFAULTS = dict(sample_rate=16000, n_fft=1024, hop=None, window="hann", band_count=8, frequency_band_maximum=8000.0,
                amplitude_minimum=0.1, amplitude_maximum=12.0, frequency_minimum=10.0, frequency_maximum=9000.0,
                max_peaks=100, local=False)


class SpectrumOut(NamedTuple):
    amplitudes: torch.Tensor        # fp32 [B, K]
    band_amplitudes: torch.Tensor   # fp32 [B, band_count]
    peak_bins: torch.Tensor         # int32 [B, max_peaks], -1 past the count
    peak_amplitudes: torch.Tensor   # fp32 [B, max_peaks], 0 past the count
    peak_counts: torch.Tensor       # int32 [B]
    power: torch.Tensor             # fp32 [B, F, K]
    image: torch.Tensor | None      # uint8 [B, H, W, 3] with ``graph``


class Tables(NamedTuple):
    """The host tables of one parameter set, as numpy arrays and scalars."""
    window: np.ndarray              # fp32 [n_fft]
    twiddle: np.ndarray             # fp32 [n_fft/2, 2]
    frequencies: np.ndarray         # fp64 [K]
    band_start: np.ndarray          # int32 [band_count + 1]
    lo: float                       # fp32 values
    hi: float
    k_lo: int
    k_hi: int


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _is_real(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)


def check_parameters(sample_rate=16000, n_fft=1024, hop=None, window="hann", band_count=8,
                     frequency_band_maximum=8000.0, amplitude_minimum=0.1, amplitude_maximum=12.0,
                     frequency_minimum=10.0, frequency_maximum=9000.0, max_peaks=100, local=False) -> None:
    """The value ranges of the rule's parameters, as ``ValueError``."""
    if not _is_int(n_fft) or n_fft not in N_FFTS:
        raise ValueError(f"spectrum: n_fft one of {N_FFTS} required, got {n_fft!r}")
    if hop is not None and (not _is_int(hop) or not 1 <= hop <= n_fft):
        raise ValueError(f"spectrum: hop an integer in 1..n_fft = {n_fft} required, got {hop!r}")
    if window not in WINDOWS:
        raise ValueError(f"spectrum: window one of {WINDOWS} required, got {window!r}")
    if not _is_real(sample_rate) or not sample_rate > 0:
        raise ValueError(f"spectrum: sample_rate > 0 required, got {sample_rate!r}")
    if not _is_int(band_count) or not 1 <= band_count <= MAX_BANDS:
        raise ValueError(f"spectrum: band_count an integer in 1..{MAX_BANDS} required, got {band_count!r}")
    if not _is_real(frequency_band_maximum) or not frequency_band_maximum > 0:
        raise ValueError(f"spectrum: frequency_band_maximum > 0 required, got {frequency_band_maximum!r}")
    if not _is_int(max_peaks) or not 1 <= max_peaks <= MAX_PEAKS:
        raise ValueError(f"spectrum: max_peaks an integer in 1..{MAX_PEAKS} required, got {max_peaks!r}")
    for name, v in (("amplitude_minimum", amplitude_minimum), ("amplitude_maximum", amplitude_maximum),
                    ("frequency_minimum", frequency_minimum), ("frequency_maximum", frequency_maximum)):
        if not _is_real(v):
            raise ValueError(f"spectrum: {name} a finite number required, got {v!r}")
    if not isinstance(local, (bool, np.bool_)):
        raise ValueError(f"spectrum: local a bool required, got {local!r}")


@functools.lru_cache(maxsize=None)
def window(kind: str, n_fft: int) -> np.ndarray:
    """The periodic window scaled by ``2 / sum(w)``, fp32 ``[n_fft]``: a sine of amplitude ``A`` at a bin
    centre reads ``A``; DC and the Nyquist bin read double."""
    t = 2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
    if kind == "hann":
        w = 0.5 - 0.5 * np.cos(t)
    elif kind == "hamming":
        w = 0.54 - 0.46 * np.cos(t)
    elif kind == "blackman":
        w = 0.42 - 0.5 * np.cos(t) + 0.08 * np.cos(2.0 * t)
    elif kind == "rect":
        w = np.ones(n_fft, np.float64)
    else:
        raise ValueError(f"spectrum: window one of {WINDOWS} required, got {kind!r}")
    w = (w * (2.0 / w.sum())).astype(np.float32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def twiddle(n_fft: int) -> np.ndarray:
    """``(cos, -sin)(2 pi j / n_fft)`` for ``j < n_fft/2``, fp32 ``[n_fft/2, 2]`` from fp64."""
    t = 2.0 * np.pi * np.arange(n_fft // 2, dtype=np.float64) / n_fft
    tw = np.stack([np.cos(t), -np.sin(t)], axis=1).astype(np.float32)
    tw.setflags(write=False)
    return tw


def frequencies(n_fft: int, rate) -> np.ndarray:
    """The bin centres, fp64 ``[K]``."""
    return np.fft.rfftfreq(int(n_fft), 1.0 / rate)


@functools.lru_cache(maxsize=None)
def tables(sample_rate=16000, n_fft=1024, window_kind="hann", band_count=8, frequency_band_maximum=8000.0,
           amplitude_minimum=0.1, amplitude_maximum=12.0, frequency_minimum=10.0, frequency_maximum=9000.0) -> Tables:
    """The host tables of one parameter set: the single definition the kernels and the reference share."""
    freq = frequencies(n_fft, sample_rate)
    edges = np.linspace(0.0, float(frequency_band_maximum), int(band_count) + 1)
    band_start = np.searchsorted(freq, edges, "left").astype(np.int32)
    lo = np.float32(amplitude_minimum)
    if float(lo) < float(amplitude_minimum):
        lo = np.nextafter(lo, np.float32(np.inf))
    hi = np.float32(amplitude_maximum)
    if float(hi) > float(amplitude_maximum):
        hi = np.nextafter(hi, np.float32(-np.inf))
    k_lo = int(np.searchsorted(freq, float(frequency_minimum), "left"))
    k_hi = int(np.searchsorted(freq, float(frequency_maximum), "right")) - 1
    for a in (freq, band_start):
        a.setflags(write=False)
    return Tables(window(window_kind, n_fft), twiddle(n_fft), freq, band_start, float(lo), float(hi), k_lo, k_hi)


def bin_pixels(freq: np.ndarray, x_max: float, width: int) -> np.ndarray:
    """The graph column of every bin, int32 ``[K]``: ``clip(int(f / x_max * (W-1)), 0, W-1)``."""
    return np.clip((np.asarray(freq, np.float64) / float(x_max) * (int(width) - 1)).astype(np.int64), 0,
                   int(width) - 1).astype(np.int32)


def frame_count(n: int, n_fft: int, hop: int) -> int:
    """``F`` of step 2."""
    return 1 if n < n_fft else 1 + (n - n_fft) // hop


def spectrum_uses_vector(audio: torch.Tensor, hop: int) -> bool:
    """Whether the ``float4`` frame pass serves this ``audio``: the first row 16-byte aligned and the
    row length and the hop multiples of 4 samples, so that every frame of every row starts aligned
    and no ``float4`` straddles the row's end; every other call runs the scalar kernel."""
    return audio.data_ptr() % 16 == 0 and audio.shape[1] % 4 == 0 and int(hop) % 4 == 0


@functools.lru_cache(maxsize=64)
def _device_tables(key, device):
    t = tables(*key)
    return (torch.from_numpy(t.window.copy()).to(device), torch.from_numpy(t.twiddle.copy()).to(device),
            torch.from_numpy(t.band_start.copy()).to(device))


@functools.lru_cache(maxsize=64)
def _device_bin_px(n_fft, sample_rate, x_max, width, device):
    return torch.from_numpy(bin_pixels(frequencies(n_fft, sample_rate), x_max, width)).to(device)


def check_graph(height, width, x_max, y_max, color) -> None:
    """The value ranges of the graph's parameters, as ``ValueError``."""
    for name, v in (("height", height), ("width", width)):
        if not _is_int(v) or not 16 <= v <= 4096:
            raise ValueError(f"spectrum_graph: {name} an integer in 16..4096 required, got {v!r}")
    for name, v in (("x_max", x_max), ("y_max", y_max)):
        if not _is_real(v) or not v > 0:
            raise ValueError(f"spectrum_graph: {name} > 0 required, got {v!r}")
    if len(color) != 3 or any(not _is_int(c) or not 0 <= c <= 255 for c in color):
        raise ValueError(f"spectrum_graph: color three integers in 0..255 required, got {color!r}")


def spectrum_graph(peak_bins: torch.Tensor, peak_amplitudes: torch.Tensor, peak_counts: torch.Tensor, *,
                   n_fft: int = 1024, sample_rate=16000, height: int = 480, width: int = 640, x_max=9000.0,
                   y_max=12.0, color=(0, 255, 0), image: torch.Tensor | None = None) -> torch.Tensor:
    """Step 8: the peaks of :func:`spectrum` as a scatter graph, uint8 ``[B, height, width, 3]``."""
    if not _is_int(n_fft) or n_fft not in N_FFTS:
        raise ValueError(f"spectrum_graph: n_fft one of {N_FFTS} required, got {n_fft!r}")
    check_graph(height, width, x_max, y_max, color)
    dev = peak_bins.device
    bin_px = _device_bin_px(int(n_fft), float(sample_rate), float(x_max), int(width), dev)
    if image is None:
        image = torch.empty(peak_bins.shape[0], int(height), int(width), 3, dtype=torch.uint8, device=dev)
    elif image.dim() != 4 or tuple(image.shape[1:]) != (int(height), int(width), 3):
        raise ValueError(f"spectrum_graph: image [B, {height}, {width}, 3] required, got {tuple(image.shape)}")
    torch.ops.aiko.spectrum_graph_out(peak_bins, peak_amplitudes, peak_counts, bin_px, float(y_max),
                                      [int(c) for c in color], image)
    return image


def spectrum(audio: torch.Tensor, *, sample_rate=16000, n_fft: int = 1024, hop: int | None = None,
             window: str = "hann", band_count: int = 8, frequency_band_maximum=8000.0, amplitude_minimum=0.1,
             amplitude_maximum=12.0, frequency_minimum=10.0, frequency_maximum=9000.0, max_peaks: int = 100,
             local: bool = False, graph=None, amplitudes: torch.Tensor | None = None,
             band_amplitudes: torch.Tensor | None = None, peak_bins: torch.Tensor | None = None,
             peak_amplitudes: torch.Tensor | None = None, peak_counts: torch.Tensor | None = None,
             power: torch.Tensor | None = None, image: torch.Tensor | None = None) -> SpectrumOut:
    """One chunk: fp32 ``[B, n]`` ``audio`` -> :class:`SpectrumOut` (the rule: this module's docstring).
    ``graph``: ``None`` (no image), or ``dict(height=480, width=640, color=(0, 255, 0))``, any key
    optional: the graph of the peaks with ``x_max = frequency_maximum`` and ``y_max =
    amplitude_maximum``, as the host ``PE_GraphXY``.  Parameters out of range are a ``ValueError``;
    shapes, dtypes, devices, overlap and ``F > 4096`` are refused by the operator."""
    check_parameters(sample_rate, n_fft, hop, window, band_count, frequency_band_maximum, amplitude_minimum,
                     amplitude_maximum, frequency_minimum, frequency_maximum, max_peaks, local)
    if audio.dim() != 2 or audio.shape[1] < 1:
        raise ValueError(f"spectrum: audio [B, n >= 1] required, got {tuple(audio.shape)}")
    hop = n_fft // 2 if hop is None else int(hop)
    gkw = None
    if graph is not None:
        gkw = dict(dict(height=480, width=640, color=(0, 255, 0)), **(graph if isinstance(graph, dict) else {}))
        check_graph(gkw["height"], gkw["width"], frequency_maximum, amplitude_maximum, gkw["color"])
    B, n = audio.shape
    F, K = frame_count(n, n_fft, hop), n_fft // 2 + 1
    dev = audio.device
    key = (float(sample_rate), int(n_fft), window, int(band_count), float(frequency_band_maximum),
           float(amplitude_minimum), float(amplitude_maximum), float(frequency_minimum), float(frequency_maximum))
    t = tables(*key)
    w, tw, band_start = _device_tables(key, dev)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    if power is None:
        if F > MAX_FRAMES:
            raise RuntimeError(f"spectrum: F = {F} frames exceed {MAX_FRAMES} per call")
        power = f32(B, F, K)
    amplitudes = f32(B, K) if amplitudes is None else amplitudes
    band_amplitudes = f32(B, int(band_count)) if band_amplitudes is None else band_amplitudes
    peak_amplitudes = f32(B, int(max_peaks)) if peak_amplitudes is None else peak_amplitudes
    if peak_bins is None:
        peak_bins = torch.empty(B, int(max_peaks), dtype=torch.int32, device=dev)
    if peak_counts is None:
        peak_counts = torch.empty(B, dtype=torch.int32, device=dev)
    for name, x, cols in (("band_amplitudes", band_amplitudes, band_count), ("peak_bins", peak_bins, max_peaks),
                          ("peak_amplitudes", peak_amplitudes, max_peaks)):
        if x.dim() != 2 or x.shape[1] != int(cols):
            raise ValueError(f"spectrum: {name} [B, {int(cols)}] required, got {tuple(x.shape)}")
    torch.ops.aiko.spectrum_out(audio, w, tw, band_start, int(n_fft), hop, float(np.float32(1.0 / F)), t.lo, t.hi,
                                t.k_lo, t.k_hi, bool(local), power, amplitudes, band_amplitudes, peak_bins,
                                peak_amplitudes, peak_counts)
    if gkw is not None:
        image = spectrum_graph(peak_bins, peak_amplitudes, peak_counts, n_fft=n_fft, sample_rate=sample_rate,
                               height=gkw["height"], width=gkw["width"], x_max=frequency_maximum,
                               y_max=amplitude_maximum, color=gkw["color"], image=image)
    else:
        image = None
    return SpectrumOut(amplitudes, band_amplitudes, peak_bins, peak_amplitudes, peak_counts, power, image)
