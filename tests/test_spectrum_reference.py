"""``spectrum_ref`` and ``spectrum_graph_ref`` (ops/reference.py), the definitions the spectrum kernels
are held to: the frame power against an fp64 FFT, tones, the chunk shapes, the host elements of
``audio_io.py`` (``PE_AudioFilter``, ``PE_AudioResampler``, ``render_xy``) as independent references,
what the scenes of spectrum_scenes.py cover, and the parameter refusals.  CPU only."""
import math
import types

import numpy as np
import pytest
import torch

import spectrum_scenes as S

RATE = S.RATE


def _ref(audio, **kw):
    from aiko_services_amd.ops.reference import spectrum_ref
    audio = torch.as_tensor(np.asarray(audio, np.float32)) if not isinstance(audio, torch.Tensor) else audio
    return spectrum_ref(audio if audio.dim() == 2 else audio[None], **kw)


def _host(cls, **params):
    """``process_frame`` of a host element of audio_io.py without a pipeline around it: its parameters
    come from ``params``."""
    me = types.SimpleNamespace(get_parameter=lambda name, default=None: (params.get(name, default), name in params),
                               counter=0)
    return types.SimpleNamespace(process_frame=lambda *args: cls.process_frame(me, *args))


@pytest.mark.parametrize("n_fft", [256, 512, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("window", ["hann", "rect"])
def test_frame_power_against_fp64(n_fft, window):
    """Per element within 8 * log2(n_fft) * 2^-24 of the frame's largest power, against np.fft.rfft in
    fp64 of the same fp32 windowed frames."""
    from aiko_services_amd.ops.reference import spectrum_power_ref
    from aiko_services_amd.ops.spectrum import window as make_window
    rng = np.random.default_rng(n_fft)
    n = n_fft + 2 * (n_fft // 2)
    noise = rng.standard_normal((2, n))
    tone = S.tones(n, [(0.5, 1000.0), (0.1, 3217.0)])
    x = np.stack([noise[0], tone + 0.01 * noise[1], 20000.0 * noise[0]]).astype(np.float32)
    v, power = spectrum_power_ref(x, n_fft, n_fft // 2, make_window(window, n_fft))
    assert v.dtype == np.float32 and power.dtype == np.float32 and power.shape == (3, 3, n_fft // 2 + 1)
    exact = np.abs(np.fft.rfft(v.astype(np.float64), axis=-1)) ** 2
    err = np.abs(power.astype(np.float64) - exact) / exact.max(axis=-1, keepdims=True)
    bound = 8 * math.log2(n_fft) * 2.0 ** -24
    print(f"n_fft {n_fft} {window}: largest error {err.max():.3e} of the frame's largest power, bound {bound:.3e}")
    assert err.max() <= bound


@pytest.mark.parametrize("window", ["hann", "hamming", "blackman", "rect"])
@pytest.mark.parametrize("n_fft", [256, 1024, 8192])
def test_a_tone_at_a_bin_centre_reads_its_amplitude(n_fft, window):
    k = n_fft // 8 + 3
    x = S.tones(3 * n_fft, [(0.5, k * RATE / n_fft)], phase=0.4)
    amp = _ref(x, n_fft=n_fft, window=window)[0][0]
    assert abs(float(amp[k]) - 0.5) <= 1e-3 and int(amp.argmax()) == k


def test_dc_reads_double():
    amp = _ref(np.full(2048, 0.25), n_fft=1024)[0][0]
    assert abs(float(amp[0]) - 0.5) <= 1e-3


def test_two_tones_are_the_first_two_local_peaks():
    n_fft = 1024
    x = S.tones(16000, [(0.3, 100 * RATE / n_fft), (0.7, 37 * RATE / n_fft)])
    rng = np.random.default_rng(0)
    x = x + 0.001 * rng.standard_normal(x.shape)
    amp, _, bins, pamp, count, _ = _ref(x, n_fft=n_fft, local=True, max_peaks=8, amplitude_minimum=0.05)
    assert int(count[0]) == 2 and bins[0, :2].tolist() == [37, 100] and bins[0, 2:].tolist() == [-1] * 6
    assert abs(float(pamp[0, 0]) - 0.7) <= 1e-3 and abs(float(pamp[0, 1]) - 0.3) <= 1e-3
    # without local the loudest bins crowd around the louder tone
    plain = _ref(x, n_fft=n_fft, max_peaks=3, amplitude_minimum=0.05)[2][0].tolist()
    assert sorted(plain) == [36, 37, 38]


def test_chunk_shapes():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 700)).astype(np.float32)
    # n < n_fft is one zero-padded frame
    short = _ref(x[:, :100], n_fft=256)
    padded = _ref(np.concatenate([x[:, :100], np.zeros((2, 156), np.float32)], axis=1), n_fft=256)
    assert short[5].shape == (2, 1, 129) and all(torch.equal(a, b) for a, b in zip(short, padded))
    # samples past the last whole frame do not matter: 700 = 256 + 4 * 100 + 44
    whole = _ref(x[:, :656], n_fft=256, hop=100)
    more = _ref(x, n_fft=256, hop=100)
    assert whole[5].shape == (2, 5, 129) and all(torch.equal(a, b) for a, b in zip(whole, more))
    # NaN and inf read as silence
    bad = x.copy()
    bad[0, 3], bad[0, 300], bad[1, 17] = np.nan, np.inf, -np.inf
    clean = bad.copy()
    clean[~np.isfinite(bad)] = 0.0
    assert all(torch.equal(a, b) for a, b in zip(_ref(bad, n_fft=256), _ref(clean, n_fft=256)))
    # full-scale PCM given unnormalised stays finite, and past full scale is clamped
    loud = np.where(rng.standard_normal((1, 8192 * 2)) > 0, 32767.0, -32767.0).astype(np.float32)
    out = _ref(loud, n_fft=8192, amplitude_maximum=1e9)
    assert all(torch.isfinite(t).all() for t in (out[0], out[1], out[3], out[5])) and float(out[5].max()) < 2.0 ** 56
    louder = _ref(np.where(loud > 0, 1e6, loud), n_fft=8192, amplitude_maximum=1e9)
    assert all(torch.equal(a, b) for a, b in zip(out, louder))
    dc = _ref(np.full((1, 8192), 1e6, np.float32), n_fft=8192, window="rect", amplitude_maximum=1e9)
    assert float(dc[0][0, 0]) == 2.0 * 32767.0


@pytest.mark.parametrize("name", S.SCENES)
def test_peaks_equal_the_host_audio_filter(name):
    """The host element's arithmetic (fp64 mask, stable argsort(-a)) on the reference's own amplitudes.
    amplitude_minimum is positive or zero in every scene, so -1 is never kept."""
    from aiko_services_amd.elements.media.audio_io import PE_AudioFilter
    from aiko_services_amd.ops.spectrum import DEFAULTS, frequencies
    s, (out, _) = S.scene(name), S.reference(name)
    kw = {**DEFAULTS, **s.kw}
    freq = frequencies(kw["n_fft"], kw["sample_rate"])
    amps = out[0].numpy().copy()
    if kw["local"]:                 # the host element has no such rule: it is given -1 where a bin is no local maximum
        a = out[0].numpy()
        inf = np.full((a.shape[0], 1), np.inf, np.float32)
        amps[~((a > np.hstack([-inf, a[:, :-1]])) & (a >= np.hstack([a[:, 1:], -inf])))] = -1.0
    host = _host(PE_AudioFilter, amplitude_minimum=kw["amplitude_minimum"], amplitude_maximum=kw["amplitude_maximum"],
                 frequency_minimum=kw["frequency_minimum"], frequency_maximum=kw["frequency_maximum"],
                 samples_maximum=kw["max_peaks"])
    for b in range(s.audio.shape[0]):
        _, want = host.process_frame(None, amps[b], freq)
        n = int(out[4][b])
        assert n == len(want["amplitudes"])
        assert np.array_equal(out[3][b, :n].numpy().astype(np.float64), want["amplitudes"])
        assert np.array_equal(freq[out[2][b, :n].numpy()], want["frequencies"])
        assert (out[2][b, n:] == -1).all() and (out[3][b, n:] == 0).all()


def test_peaks_with_thresholds_that_are_not_fp32_values_and_a_tie():
    from aiko_services_amd.elements.media.audio_io import PE_AudioFilter
    from aiko_services_amd.ops.spectrum import frequencies, tables
    x = S.scene("ties").audio
    amp = _ref(x, n_fft=256, hop=256, window="rect")[0]
    freq = frequencies(256, RATE)
    a0 = float(amp[0, 5])                                          # every bin of row 0 reads this
    assert (amp[0] == amp[0, 5]).all()
    up, down = float(np.nextafter(np.float32(a0), np.float32(np.inf))), float(np.nextafter(np.float32(a0), np.float32(0)))
    cases = [((a0 + up) / 2, 12.0, 0), ((a0 + down) / 2, 12.0, 100), (0.1, (a0 + down) / 2, 0), (0.1, (a0 + up) / 2, 100),
             (a0, a0, 100), (0.1, 0.3, 0)]
    for a_min, a_max, want_count in cases:
        kw = dict(amplitude_minimum=a_min, amplitude_maximum=a_max)
        t = tables(float(RATE), 256, "rect", 8, 8000.0, a_min, a_max, 10.0, 9000.0)
        assert np.float32(t.lo) == t.lo and np.float32(t.hi) == t.hi and t.lo >= a_min and t.hi <= a_max
        out = _ref(x[:1], n_fft=256, hop=256, window="rect", max_peaks=100, **kw)
        _, want = _host(PE_AudioFilter, samples_maximum=100, **kw).process_frame(None, amp[0].numpy(), freq)
        n = int(out[4][0])
        assert n == want_count == len(want["amplitudes"]), (a_min, a_max)
        assert np.array_equal(freq[out[2][0, :n].numpy()], want["frequencies"])       # ties: the lower bin first
        assert out[2][0, :n].tolist() == list(range(1, 1 + n))


@pytest.mark.parametrize("name", S.SCENES)
def test_bands_against_the_host_audio_resampler(name):
    """Each band within m * 2^-24 (relative) of the host element's fp64 sums, m the band's bin count."""
    from aiko_services_amd.elements.media.audio_io import PE_AudioResampler
    from aiko_services_amd.ops.spectrum import DEFAULTS, frequencies
    s, (out, _) = S.scene(name), S.reference(name)
    kw = {**DEFAULTS, **s.kw}
    freq = frequencies(kw["n_fft"], kw["sample_rate"])
    host = _host(PE_AudioResampler, band_count=kw["band_count"], frequency_maximum=kw["frequency_band_maximum"])
    m = np.diff(_band_start(kw))
    assert (m >= 0).all()
    for b in range(s.audio.shape[0]):
        _, want = host.process_frame(None, out[0][b].numpy(), freq)
        got = out[1][b].numpy().astype(np.float64)
        assert np.all(np.abs(got - want["amplitudes"]) <= m * 2.0 ** -24 * want["amplitudes"]), name
        assert (got[m == 0] == 0).all()


def test_graph_equals_render_xy():
    from aiko_services_amd.elements.media.audio_io import render_xy
    from aiko_services_amd.ops.reference import spectrum_graph_ref
    from aiko_services_amd.ops.spectrum import frequencies
    for H, W, color in ((48, 64, (0, 255, 0)), (16, 16, (9, 8, 7)), (480, 640, (0, 255, 0))):
        bins, amps, counts = S.graph_points(H, W)
        freq = frequencies(256, RATE)
        got = spectrum_graph_ref(bins, amps, counts, n_fft=256, height=H, width=W, x_max=7000.0, y_max=12.0, color=color)
        assert got.dtype == torch.uint8 and got.shape == (3, H, W, 3)
        for b in range(3):
            n = int(counts[b])
            want = render_xy(freq[bins[b, :n].numpy()], amps[b, :n].numpy(), W, H, 7000.0, 12.0, color)
            assert np.array_equal(got[b].numpy(), want), (H, W, b)
        corners = got[0][[0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]]
        assert (corners == torch.tensor(color, dtype=torch.uint8)).all()        # dots clipped into all four corners
    for name in S.SCENES:
        s, (out, image) = S.scene(name), S.reference(name)
        if s.graph is None:
            continue
        g = S.graph_kw(s)
        freq = frequencies(g["n_fft"], g["sample_rate"])
        for b in range(s.audio.shape[0]):
            n = int(out[4][b])
            want = render_xy(freq[out[2][b, :n].numpy()], out[3][b, :n].numpy(), g["width"], g["height"], g["x_max"],
                             g["y_max"], g.get("color", (0, 255, 0)))
            assert np.array_equal(image[b].numpy(), want), (name, b)


def test_scenes_cover_what_they_claim():
    from aiko_services_amd.ops.spectrum import DEFAULTS, frame_count, spectrum_uses_vector
    seen = set()
    for name in S.SCENES:
        s, (out, _) = S.scene(name), S.reference(name)
        kw = {**DEFAULTS, **s.kw}
        B, n = s.audio.shape
        hop = kw["hop"] or kw["n_fft"] // 2
        assert frame_count(n, kw["n_fft"], hop) == s.frames == out[5].shape[1]
        assert out[5].shape == (B, s.frames, kw["n_fft"] // 2 + 1) and all(torch.isfinite(t).all() for t in out)
        counts = out[4].tolist()
        seen.add(("n_fft", kw["n_fft"], "B", B))
        seen.add(("F", s.frames))
        seen.add(("vector", spectrum_uses_vector(s.audio, hop)))
        seen.add(("bands", kw["band_count"], "empty", bool((np.diff(_band_start(kw)) == 0).any())))
        seen.update(("peaks", kw["max_peaks"], "full" if c == kw["max_peaks"] else "none" if c == 0 else "some",
                     "local", kw["local"]) for c in counts)
    for need in (("n_fft", 256, "B", 1), ("n_fft", 256, "B", 3), ("n_fft", 8192, "B", 1), ("n_fft", 8192, "B", 3),
                 ("F", 1), ("F", 2), ("F", 5), ("vector", True), ("vector", False), ("bands", 1, "empty", False),
                 ("bands", 64, "empty", True), ("peaks", 1, "full", "local", True), ("peaks", 128, "full", "local", False),
                 ("peaks", 128, "some", "local", False), ("peaks", 128, "some", "local", True),
                 ("peaks", 128, "none", "local", False)):
        assert need in seen, (need, sorted(map(str, seen)))
    # the scalar scene: n odd, hop % 4 != 0
    odd = S.scene("odd")
    assert odd.audio.shape[1] % 2 == 1 and odd.kw["hop"] % 4 != 0
    ties = S.reference("ties")[0]
    assert all((ties[0][b] == ties[0][b, 0]).all() for b in range(3)) and ties[2][0].tolist() == list(range(1, 129))
    assert S.reference("ties_local")[0][2][0, :2].tolist() == [0, -1]


def _band_start(kw):
    from aiko_services_amd.ops.spectrum import tables
    return tables(float(kw["sample_rate"]), kw["n_fft"], kw["window"], kw["band_count"],
                  float(kw["frequency_band_maximum"]), float(kw["amplitude_minimum"]), float(kw["amplitude_maximum"]),
                  float(kw["frequency_minimum"]), float(kw["frequency_maximum"])).band_start


def test_tables():
    from aiko_services_amd.ops.spectrum import bin_pixels, frequencies, tables, twiddle, window
    for kind in ("hann", "hamming", "blackman", "rect"):
        w = window(kind, 512)
        assert w.dtype == np.float32 and w.shape == (512,) and abs(float(w.astype(np.float64).sum()) - 2.0) < 1e-5
    assert window("hann", 256)[0] == 0.0 and window("rect", 256)[7] == np.float32(2.0 / 256)
    tw = twiddle(1024)
    assert tw.dtype == np.float32 and tw.shape == (512, 2) and tw[0].tolist() == [1.0, -0.0] and tw[256, 1] == -1.0
    assert np.array_equal(frequencies(1024, 16000), np.fft.rfftfreq(1024, 1 / 16000))
    t = tables()
    assert t.band_start.tolist() == [0, 64, 128, 192, 256, 320, 384, 448, 512]       # bin 512 (8000 Hz) is in no band
    assert (t.k_lo, t.k_hi) == (1, 512) and t.lo == float(np.float32(0.1)) and t.hi == 12.0
    assert tables() is t
    px = bin_pixels(frequencies(256, 16000), 4000.0, 64)
    assert px.dtype == np.int32 and px[0] == 0 and px[64] == 63 and px[128] == 63 and px[32] == 31


def test_refusals():
    from aiko_services_amd.ops.reference import spectrum_graph_ref
    from aiko_services_amd.ops.spectrum import check_graph, check_parameters
    check_parameters()
    check_parameters(n_fft=8192, hop=8192, band_count=64, max_peaks=128, window="rect", local=True)
    for match, kw in (("n_fft", dict(n_fft=1000)), ("n_fft", dict(n_fft=128)), ("n_fft", dict(n_fft=16384)),
                      ("n_fft", dict(n_fft=1024.0)), ("hop", dict(hop=0)), ("hop", dict(hop=1025)),
                      ("hop", dict(hop=2.5)), ("window", dict(window="kaiser")), ("band_count", dict(band_count=0)),
                      ("band_count", dict(band_count=65)), ("frequency_band_maximum", dict(frequency_band_maximum=0)),
                      ("max_peaks", dict(max_peaks=0)), ("max_peaks", dict(max_peaks=129)),
                      ("max_peaks", dict(max_peaks=True)), ("sample_rate", dict(sample_rate=0)),
                      ("amplitude_minimum", dict(amplitude_minimum=float("nan"))),
                      ("frequency_maximum", dict(frequency_maximum=float("inf"))), ("local", dict(local=1))):
        with pytest.raises(ValueError, match=match):
            check_parameters(**kw)
        with pytest.raises(ValueError, match=match):
            _ref(np.zeros((1, 2048), np.float32), **kw)
    with pytest.raises(ValueError, match="F = 4097"):
        _ref(np.zeros((1, 256 + 4096), np.float32), n_fft=256, hop=1)
    assert _ref(np.zeros((1, 256 + 4095), np.float32), n_fft=256, hop=1)[5].shape == (1, 4096, 129)
    check_graph(16, 4096, 1.0, 1e-3, (0, 0, 255))
    for match, args in (("height", (15, 64, 1.0, 1.0, (0, 255, 0))), ("width", (48, 4097, 1.0, 1.0, (0, 255, 0))),
                        ("x_max", (48, 64, 0.0, 1.0, (0, 255, 0))), ("y_max", (48, 64, 1.0, -1.0, (0, 255, 0))),
                        ("color", (48, 64, 1.0, 1.0, (0, 256, 0))), ("color", (48, 64, 1.0, 1.0, (0, 255)))):
        with pytest.raises(ValueError, match=match):
            check_graph(*args)
    with pytest.raises(ValueError, match="height"):
        spectrum_graph_ref(*S.graph_points(), n_fft=256, height=8, width=64)
