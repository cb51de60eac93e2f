"""Chunks for the spectrum tests, shared by the CPU tests of the reference and the GPU tests of the
kernels: small seeded signals that between them take every path of the rule, each with the
parameters it is analysed with and, for some, a graph.  ``reference(name)`` computes a scene's
reference once."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

RATE = 16000


class Scene(NamedTuple):
    audio: torch.Tensor            # fp32 [B, n]
    kw: dict                       # the parameters of ops.spectrum.spectrum
    graph: dict | None             # height, width (and color) of the graph, or None
    frames: int                    # the F the scene is built for


def tones(n, parts, rate=RATE, phase=0.0):
    """A sum of sines: ``parts`` is ``[(amplitude, hertz), ...]``; fp64 ``[n]``."""
    t = np.arange(n, dtype=np.float64) / rate
    return sum(a * np.sin(2.0 * np.pi * f * t + phase) for a, f in parts)


def _mix(B, n, seed, rate=RATE, noise=0.02):
    """``B`` streams of two or three tones of different loudness over a little noise."""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(B):
        parts = [(float(rng.uniform(0.2, 2.0)), float(rng.uniform(0.02, 0.45)) * rate) for _ in range(2 + b % 2)]
        rows.append(tones(n, parts, rate, phase=0.3 * b) + noise * rng.standard_normal(n))
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def _impulses(B, n, n_fft, hop, seed):
    """One impulse at the start of every frame: under the rect window every bin of a frame then has
    the same power, so every amplitude of a row ties with every other."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, n), np.float32)
    for f in range(1 + (n - n_fft) // hop):
        x[:, f * hop] = rng.uniform(200.0, 1200.0, B).astype(np.float32)
    return torch.from_numpy(x)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    if name == "short":             # n < n_fft: one zero-padded frame; 64 bands, most of them empty; all 128 peaks asked for
        return Scene(_mix(3, 100, 1), dict(n_fft=256, band_count=64, frequency_band_maximum=1000.0, max_peaks=128,
                                           amplitude_minimum=0.05), dict(height=16, width=16), 1)
    if name == "odd":               # F = 2, hop % 4 != 0, n odd: rows 1 and 2 unaligned, the scalar pass
        return Scene(_mix(3, 363, 2), dict(n_fft=256, hop=101, band_count=1, max_peaks=1, local=True),
                     dict(height=48, width=64, color=(255, 0, 7)), 2)
    if name == "overlap":           # F = 5 at hop = n_fft / 4, the float4 pass
        return Scene(_mix(1, 512, 3), dict(n_fft=256, hop=64, band_count=8, max_peaks=100, local=True,
                                           window="blackman"), dict(height=48, width=64), 5)
    if name == "ties":              # every amplitude of a row ties: ties go to the lower bin; kept = 128 = max_peaks
        return Scene(_impulses(3, 512, 256, 256, 4), dict(n_fft=256, hop=256, window="rect", max_peaks=128,
                                                          band_count=64, frequency_band_maximum=8000.0), None, 2)
    if name == "ties_local":        # ... and with local only bin 0 survives: no other bin is above its left neighbour
        return Scene(_impulses(1, 512, 256, 256, 4), dict(n_fft=256, hop=256, window="rect", max_peaks=128,
                                                          frequency_minimum=0.0, local=True), None, 2)
    if name == "none":              # nothing kept: silence with NaN and inf in it
        x = torch.zeros(3, 300)
        x[0, 5], x[1, 7], x[2, 299] = float("nan"), float("inf"), -float("inf")
        return Scene(x, dict(n_fft=256, hop=44, band_count=64, max_peaks=128), dict(height=16, width=16), 2)
    if name == "chunk48k":          # the host chain's 0.1 s at 48 kHz: one zero-padded frame of 8192
        return Scene(_mix(3, 4800, 5, rate=48000), dict(sample_rate=48000, n_fft=8192, max_peaks=128, local=True,
                                                        frequency_maximum=20000.0, band_count=64,
                                                        frequency_band_maximum=30000.0),
                     dict(height=48, width=64), 1)
    if name == "big":               # 8192, F = 5 overlapping, every bin kept: the whole sort, all of the LDS
        x = _mix(1, 8192 + 4 * 2048, 6, noise=0.5) * 40.0
        return Scene(x, dict(n_fft=8192, hop=2048, window="hamming", max_peaks=128, amplitude_minimum=0.0,
                             amplitude_maximum=1e9, frequency_minimum=0.0, frequency_maximum=1e9, band_count=1,
                             frequency_band_maximum=8000.5), None, 5)
    if name == "loud":              # unnormalised PCM at full scale and past it, on the scalar pass
        x = _mix(1, 1030, 7) * 40000.0
        return Scene(x, dict(n_fft=512, hop=259, amplitude_maximum=1e6, max_peaks=16, local=True), None, 3)
    raise KeyError(name)


SCENES = ("short", "odd", "overlap", "ties", "ties_local", "none", "chunk48k", "big", "loud")
NAMES = ("amplitudes", "band_amplitudes", "peak_bins", "peak_amplitudes", "peak_counts", "power")


def graph_kw(s: Scene) -> dict:
    """The parameters of ``spectrum_graph`` / ``spectrum_graph_ref`` for a scene with a graph."""
    kw = s.kw
    return dict(n_fft=kw["n_fft"], sample_rate=kw.get("sample_rate", RATE), x_max=kw.get("frequency_maximum", 9000.0),
                y_max=kw.get("amplitude_maximum", 12.0), **s.graph)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """``(the six outputs of spectrum_ref, the image of spectrum_graph_ref or None)``, computed once."""
    from aiko_services_amd.ops.reference import spectrum_graph_ref, spectrum_ref
    s = scene(name)
    out = spectrum_ref(s.audio, **s.kw)
    image = spectrum_graph_ref(out[2], out[3], out[4], **graph_kw(s)) if s.graph else None
    return out, image


def graph_points(H=48, W=64, n_fft=256, y_max=12.0):
    """Peaks for the graph alone: dots clipped at all four borders, an amplitude past ``y_max``, one of
    0, two on the same pixel, and a row with no peak: ``(peak_bins, peak_amplitudes, peak_counts)``."""
    K = n_fft // 2 + 1
    bins = torch.full((3, 8), -1, dtype=torch.int32)
    amps = torch.zeros(3, 8)
    bins[0, :7] = torch.tensor([0, K - 1, 0, K - 1, K // 2, K // 2, 3], dtype=torch.int32)
    amps[0, :7] = torch.tensor([0.0, y_max * 1.5, y_max * 1.5, 0.0, y_max / 3, y_max / 3, y_max * 0.999])
    bins[1, :2] = torch.tensor([K - 1, 0], dtype=torch.int32)
    amps[1, :2] = torch.tensor([0.0, 1e6])
    return bins, amps, torch.tensor([7, 2, 0], dtype=torch.int32)
