"""The spectrum kernels (``ops.spectrum.spectrum`` / ``spectrum_graph``, spectrum_ops.hip) against the
CPU references, bit for bit in all six outputs and the image, on the scenes of spectrum_scenes.py;
between guard bands; under hipGraph replay; the square root's rounding; the limits of the launch;
then the element in the example pipeline against direct calls."""
import json
import queue
from pathlib import Path

import numpy as np
import pytest
import torch

import spectrum_scenes as S
from kernel_guard import guarded

pytestmark = pytest.mark.gpu

NAMES = S.NAMES


def _assert_out(got, want, where):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, f"{where}: {name} {g.dtype} {tuple(g.shape)}"
        if g.dtype == torch.float32:                        # bit for bit: the sign of a zero and NaN would show
            g, w = g.view(torch.int32), w.view(torch.int32)
        bad = (g != w).nonzero()
        assert not len(bad), f"{where}: {name} differs at {bad[0].tolist()} ({len(bad)} elements)"


def _place(audio, offset):
    """``audio`` on the device, contiguous, ``offset`` floats past a 16-byte boundary."""
    flat = torch.empty(audio.numel() + 4, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + audio.numel()].view(audio.shape)
    view.copy_(audio)
    return view


@pytest.mark.parametrize("name", S.SCENES)
def test_scenes_equal_the_reference(native, name):
    from aiko_services_amd.ops.spectrum import spectrum, spectrum_uses_vector
    s, (want, want_image) = S.scene(name), S.reference(name)
    hop = s.kw.get("hop") or s.kw["n_fft"] // 2
    for offset in (0, 1):
        audio = _place(s.audio, offset)
        if offset:
            assert not spectrum_uses_vector(audio, hop)
        got = spectrum(audio, graph=s.graph, **s.kw)
        torch.cuda.synchronize()
        _assert_out(got[:6], want, f"{name}, offset {offset}")
        if s.graph:
            assert got.image.dtype == torch.uint8 and torch.equal(got.image.cpu(), want_image), f"{name}: image"
        else:
            assert got.image is None


def test_graph_alone(native):
    """Dots clipped at all four borders, amplitudes past y_max, a stream without peaks; 16 x 16, 48 x 64
    and a width whose rows are not whole words."""
    from aiko_services_amd.ops.reference import spectrum_graph_ref
    from aiko_services_amd.ops.spectrum import spectrum_graph
    for H, W, color in ((16, 16, (9, 8, 7)), (48, 64, (0, 255, 0)), (35, 27, (255, 255, 255))):
        bins, amps, counts = S.graph_points(H, W)
        kw = dict(n_fft=256, height=H, width=W, x_max=7000.0, y_max=12.0, color=color)
        want = spectrum_graph_ref(bins, amps, counts, **kw)
        got = spectrum_graph(bins.cuda(), amps.cuda(), counts.cuda(), **kw)
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), want), (H, W)


@pytest.mark.parametrize("name", ["odd", "chunk48k"])
def test_guard_bands_and_every_element_written(native, name):
    from aiko_services_amd.ops.spectrum import DEFAULTS, spectrum
    s, (want, want_image) = S.scene(name), S.reference(name)
    kw = {**DEFAULTS, **s.kw}
    B, n = s.audio.shape
    K, F = kw["n_fft"] // 2 + 1, s.frames
    checks = []

    def g(shape, dtype, values=None, name="", poison=None):
        view, check = guarded(shape, dtype, "cuda", values=values, name=name, poison=poison)
        checks.append(check)
        return view

    audio = g((B, n), torch.float32, s.audio, "audio")
    outs = dict(amplitudes=g((B, K), torch.float32, name="amplitudes"),
                band_amplitudes=g((B, kw["band_count"]), torch.float32, name="band_amplitudes"),
                peak_bins=g((B, kw["max_peaks"]), torch.int32, name="peak_bins"),
                peak_amplitudes=g((B, kw["max_peaks"]), torch.float32, name="peak_amplitudes"),
                peak_counts=g((B,), torch.int32, name="peak_counts"), power=g((B, F, K), torch.float32, name="power"),
                image=g((B, s.graph["height"], s.graph["width"], 3), torch.uint8, name="image", poison=0xFF))
    got = spectrum(audio, graph=s.graph, **s.kw, **outs)
    torch.cuda.synchronize()
    for check in checks:
        check()
    _assert_out(got[:6], want, f"{name}, guarded")           # equal to a finite reference: no NaN poison is left
    assert torch.equal(got.image.cpu(), want_image)
    assert all(got[i].data_ptr() == outs[k].data_ptr() for i, k in enumerate(NAMES))
    assert got.image.data_ptr() == outs["image"].data_ptr() and torch.equal(audio.cpu(), s.audio)


def test_graph_replay_on_changed_input(native):
    from aiko_services_amd.ops.reference import spectrum_graph_ref, spectrum_ref
    from aiko_services_amd.ops.spectrum import spectrum
    kw = dict(n_fft=256, hop=64, band_count=8, max_peaks=16, local=True)
    gk = dict(height=16, width=16)
    inputs = [S._mix(3, 512, seed) for seed in (11, 12, 13)]
    audio = inputs[0].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = spectrum(audio, graph=gk, **kw)
    torch.cuda.current_stream().wait_stream(side)
    bufs = dict(zip((*NAMES, "image"), out))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        spectrum(audio, graph=gk, **kw, **bufs)
    for x in inputs[1:]:
        audio.copy_(x)
        for t in bufs.values():                               # poison: every element must be rewritten
            t.view(torch.uint8).fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        want = spectrum_ref(x, **kw)
        _assert_out(out[:6], want, "replay")
        image = spectrum_graph_ref(want[2], want[3], want[4], n_fft=256, x_max=9000.0, y_max=12.0, **gk)
        assert torch.equal(out.image.cpu(), image)


def test_square_root_is_correctly_rounded(native):
    """Amplitudes over 80 octaves, subnormal powers among them: each equals the fp64 square root of
    the fp32 mean power rounded once (exact for fp32: 53 >= 2 * 24 + 2), and the reference."""
    from aiko_services_amd.ops.reference import spectrum_ref
    from aiko_services_amd.ops.spectrum import spectrum
    rng = np.random.default_rng(21)
    B = 64
    scale = 2.0 ** np.linspace(-68.0, 14.0, B)
    x = torch.from_numpy((rng.standard_normal((B, 512)) * scale[:, None]).astype(np.float32))
    kw = dict(n_fft=256, hop=128, amplitude_minimum=0.0, amplitude_maximum=1e9, max_peaks=8)
    got = spectrum(x.cuda(), **kw)
    torch.cuda.synchronize()
    _assert_out(got[:6], spectrum_ref(x, **kw), "sweep")
    power = got.power.cpu().numpy()
    assert power.shape[1] == 3
    acc = (power[:, 0] + power[:, 1]) + power[:, 2]
    mean = acc * np.float32(1.0 / 3)
    assert mean.dtype == np.float32
    want = np.sqrt(mean.astype(np.float64)).astype(np.float32)
    amp = got.amplitudes.cpu().numpy()
    assert np.array_equal(amp.view(np.int32), want.view(np.int32))
    roots = want.astype(np.float64) ** 2 == mean.astype(np.float64)
    assert roots.mean() < 0.01                                # hardly a perfect square among them
    assert (mean[mean > 0] < 1.17549435e-38).any() and (mean > 1e6).any()


def test_refusals(native):
    from aiko_services_amd.ops.spectrum import spectrum, spectrum_graph
    audio = torch.zeros(2, 1024, device="cuda")

    def refuse(match, audio=audio, error=RuntimeError, **kw):
        with pytest.raises(error, match=match):
            spectrum(audio, **{"n_fft": 256, **kw})

    refuse("F = 4097", audio=torch.zeros(1, 256 + 4096, device="cuda"), hop=1)
    refuse("audio fp32", audio=audio.half())
    refuse("audio fp32", audio=torch.zeros(2, 2048, device="cuda")[:, ::2])
    refuse("audio", audio=torch.zeros(2, 0, device="cuda"), error=ValueError)
    refuse("GPU tensor", power=torch.empty(2, 7, 129))
    refuse("power fp32", power=torch.empty(2, 6, 129, device="cuda"))
    refuse("amplitudes fp32", amplitudes=torch.empty(2, 128, device="cuda"))
    refuse("peak_counts int32", peak_counts=torch.empty(2, dtype=torch.int64, device="cuda"))
    refuse("peak_bins", error=ValueError, peak_bins=torch.empty(2, 50, dtype=torch.int32, device="cuda"))
    shared = torch.zeros(400, device="cuda")
    refuse("peak_amplitudes and band_amplitudes overlap", peak_amplitudes=shared[:200].view(2, 100),
           band_amplitudes=shared[196:212].view(2, 8))
    refuse("power and audio overlap", audio=shared[:200].view(2, 100), power=shared[100:358].view(2, 1, 129))
    refuse("n_fft", error=ValueError, n_fft=300)
    refuse("hop", error=ValueError, hop=257)
    refuse("max_peaks", error=ValueError, max_peaks=129)
    refuse("height", error=ValueError, graph=dict(height=8))
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device="cuda")  # noqa: E731
    with pytest.raises(RuntimeError, match="16 <= H, W <= 4096"):
        torch.ops.aiko.spectrum_graph_out(i32(1, 4), torch.zeros(1, 4, device="cuda"), i32(1), i32(129), 12.0,
                                          [0, 255, 0], torch.empty(1, 8, 64, 3, dtype=torch.uint8, device="cuda"))
    both = torch.zeros(16 * 16 * 3, dtype=torch.uint8, device="cuda")       # the image over its own peaks
    with pytest.raises(RuntimeError, match="image and peak_amplitudes overlap"):
        torch.ops.aiko.spectrum_graph_out(i32(1, 4), both[:16].view(torch.float32).view(1, 4), i32(1), i32(129), 12.0,
                                          [0, 255, 0], both.view(1, 16, 16, 3))
    with pytest.raises(RuntimeError, match="max_peaks"):
        spectrum_graph(i32(1, 129), torch.zeros(1, 129, device="cuda"), i32(1), n_fft=256, height=16, width=16)
    # the extremes inside the limits: 4096 frames of one stream
    out = spectrum(torch.zeros(1, 256 + 4095, device="cuda"), n_fft=256, hop=1, max_peaks=1, band_count=64)
    torch.cuda.synchronize()
    assert out.power.shape == (1, 4096, 129) and not out.power.any() and out.peak_counts.tolist() == [0]


# ---- the example pipeline -------------------------------------------------------------------

EXAMPLE = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/speech/pipeline_spectrum_gpu.json"
PIPE_B, PIPE_CHUNKS = 2, 3
PIPE_KW = dict(n_fft=256, hop=128, band_count=8, samples_maximum=12, local=True, width=64, height=48)


def _definition(lanes):
    d = json.loads(EXAMPLE.read_text())
    assert d["graph"] == ["(AudioChunks AudioResample AudioSpectrum SpectrumResults JpegEncode)"]
    d["parameters"]["gpu_lanes"] = lanes
    by_name = {e["name"]: e for e in d["elements"]}
    by_name["AudioChunks"]["input"] = [{"name": "audio_samples", "type": "ndarray"}]
    assert by_name["AudioSpectrum"]["parameters"]["graph"] is True
    by_name["AudioSpectrum"]["parameters"].update(PIPE_KW)
    return d


def _pcm_chunks():
    """Three 0.1 s chunks of 48 kHz stereo int16 for two streams: two tones each, moving between chunks."""
    out = []
    for t in range(PIPE_CHUNKS):
        rows = [S.tones(4800, [(0.6, 500.0 + 700.0 * t + 300.0 * b), (0.25, 3000.0 + 500.0 * b)], rate=48000)
                for b in range(PIPE_B)]
        pcm = np.round(np.stack(rows) * 32767.0).clip(-32768, 32767).astype(np.int16)
        out.append(np.ascontiguousarray(np.stack([pcm, pcm], axis=2)))        # [B, n, 2]
    return out


def _run_pipeline(lanes):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<spectrum>", parse_pipeline_definition_dict(_definition(lanes)), None, None, "c",
                                     [], 0, None, 60, queue_response=q)
    p.response_swag = True                     # the whole swag comes back, device tensors included
    element = p.pipeline_graph.get_node("AudioSpectrum").element
    inner, seen = element.process_frame, []

    def spy(stream, audio, *args, **kw):
        seen.append(audio.clone())
        event, swag = inner(stream, audio, *args, **kw)
        if "images" in swag:
            seen_images.append(swag["images"].clone())    # JpegEncode replaces ``images`` in the swag
        return event, swag

    seen_images = []
    element.process_frame = spy
    outs = []
    for i, chunk in enumerate(_pcm_chunks()):
        p.process_frame({"stream_id": "c", "frame_id": i}, {"audio_samples": chunk})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        torch.cuda.synchronize()               # buffers are reused per lane: copy before the next frame
        host = swag["spectrum"].wait()
        assert all(t.is_pinned() for t in host.values())
        for key in ("amplitudes", "band_amplitudes", "peak_bins", "peak_amplitudes", "peak_counts"):
            assert host[key].device.type == "cpu" and torch.equal(host[key], swag[key].cpu()), key
        assert swag["nbytes"].shape == (PIPE_B,) and (swag["nbytes"] > 0).all()   # JpegEncode took the graph images
        outs.append({"source": seen[i], "graph": seen_images[i], "host": {k: v.clone() for k, v in host.items()},
                     **{k: swag[k].clone() for k in NAMES}})
    assert p.share["gpu_lanes"] == lanes and len(seen) == PIPE_CHUNKS
    element.process_frame = inner
    return outs, p


def test_spectrum_pipeline_matches_direct_calls(native):
    from aiko_services_amd.elements.gpu.spectrum import to_host_spectrum
    from aiko_services_amd.ops.reference import spectrum_graph_ref, spectrum_ref
    from aiko_services_amd.ops.spectrum import frequencies, spectrum
    from aiko_services_amd.pipeline.stream import StreamEvent
    one, p = _run_pipeline(1)
    kw = dict(n_fft=256, hop=128, band_count=8, max_peaks=12, local=True)
    gk = dict(height=48, width=64)
    tops = []
    for i, o in enumerate(one):
        assert o["source"].shape == (PIPE_B, 1600) and o["source"].dtype == torch.float32
        got = spectrum(o["source"], graph=gk, **kw)
        want = spectrum_ref(o["source"].cpu(), **kw)
        torch.cuda.synchronize()
        _assert_out(got[:6], want, f"direct, chunk {i}")
        _assert_out([o[k] for k in NAMES], want, f"pipeline, chunk {i}")
        image = spectrum_graph_ref(want[2], want[3], want[4], n_fft=256, x_max=9000.0, y_max=12.0, **gk)
        assert torch.equal(o["graph"].cpu(), image) and torch.equal(got.image.cpu(), image)
        for b in range(PIPE_B):
            pts = to_host_spectrum(o["host"], b, n_fft=256)
            n = int(want[4][b])
            assert pts["amplitudes"].dtype == np.float64 and len(pts["amplitudes"]) == n >= 2
            assert np.array_equal(pts["frequencies"], frequencies(256, 16000)[want[2][b, :n].numpy()])
        tops.append(frequencies(256, 16000)[want[2][:, 0].numpy()].tolist())
    # the loudest point follows the louder tone: 500 + 700 t + 300 b Hz, within a bin of 62.5 Hz
    for t, row in enumerate(tops):
        for b, f in enumerate(row):
            assert abs(f - (500.0 + 700.0 * t + 300.0 * b)) <= 62.5, (t, b, f)
    two, _ = _run_pipeline(2)
    for a, b in zip(one, two):
        for key in ("source", "graph", *NAMES):
            assert torch.equal(a[key], b[key]), key
    element = p.pipeline_graph.get_node("AudioSpectrum").element
    for bad, text in ((torch.zeros(PIPE_B, 320, device="cuda").half(), "audio fp32"), (None, "audio fp32"),
                      (torch.zeros(PIPE_B, 320), "audio fp32"),
                      (torch.zeros(1, 256 + 128 * 4096, device="cuda"), "4097 frames")):
        event, out = element.process_frame(None, bad)
        assert event == StreamEvent.ERROR and text in out["diagnostic"], out
