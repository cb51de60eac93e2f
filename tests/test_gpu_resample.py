"""Raw PCM in on the MI355X (``resample_ops.hip``): every geometry against ``resample_ref`` bit for
bit, the vector and the scalar path, extremes, streaming with a carried history, guard bands,
hipGraph replay, refusals, and AudioChunks (pcm16) / AudioResample / the 48 kHz WAV example."""
import json
import queue
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

from kernel_guard import guarded

pytestmark = pytest.mark.gpu

_CASES = {}


def case(rate, channels, n_in, batch=2, dtype=torch.int16, seed=0, hist="random"):
    """(pcm, hist, filt, L, M, reference out, reference hist_out) on the host, made once per case."""
    key = (rate, channels, n_in, batch, dtype, seed, hist)
    if key not in _CASES:
        from aiko_services_amd.ops import audio as A
        from aiko_services_amd.ops.reference import resample_ref
        filt, L, M = A.resample_filter(rate, 16000)
        T = filt.shape[1]
        g = torch.Generator().manual_seed(rate + 1000 * channels + n_in + batch + seed)
        if dtype == torch.int16:
            pcm = torch.randint(-32768, 32768, (batch, n_in, channels), generator=g).to(torch.int16)
        else:
            pcm = torch.rand(batch, n_in, channels, generator=g) * 2 - 1
        h = torch.rand(batch, T - 1, generator=g) * 2 - 1 if hist == "random" else torch.zeros(batch, T - 1)
        _CASES[key] = (pcm, h, filt, L, M, *resample_ref(pcm, h, filt, L, M))
    return _CASES[key]


def run(pcm, hist, filt, L, M):
    """The op on device copies of the operands, into poisoned outputs."""
    from aiko_services_amd.ops import audio as A
    B, n_in, _ = pcm.shape
    out = torch.full((B, n_in * L // M), float("nan"), device="cuda")
    hist_out = torch.full((B, filt.shape[1] - 1), float("nan"), device="cuda")
    got = A.resample(pcm, hist.cuda(), filt.cuda(), L, M, out=out, hist_out=hist_out)
    torch.cuda.synchronize()
    assert got[0] is out and got[1] is hist_out
    return out.cpu(), hist_out.cpu()


def misaligned(pcm):
    """A contiguous device copy that starts one element into an allocation."""
    buf = torch.empty(pcm.numel() + 8, dtype=pcm.dtype, device="cuda")
    view = buf[1:1 + pcm.numel()].view(pcm.shape)
    view.copy_(pcm)
    assert view.is_contiguous() and view.data_ptr() % 16 == pcm.element_size()
    return view


# ---- geometry -------------------------------------------------------------------------------

def _tile():
    from aiko_services_amd.ops.audio import RESAMPLE_TILE
    return RESAMPLE_TILE


# (name, rate, channels, n_in or a function of the tile, batch, dtype, vector path)
GEOMETRY = [
    ("tile+1", 48000, 1, lambda t: 3 * (t + 1), 2, torch.int16, False),
    ("2tiles+5", 48000, 1, lambda t: 3 * (2 * t + 5), 2, torch.int16, False),
    ("tile+8", 48000, 1, lambda t: 3 * (t + 8), 2, torch.int16, True),
    ("441-phases", 44100, 2, 441 * 8, 2, torch.int16, True),
    ("up-c3", 8000, 3, 40, 2, torch.int16, False),
    ("96k", 96000, 1, 6 * 50, 2, torch.int16, False),
    ("equal-c2", 16000, 2, 50, 2, torch.int16, False),
    ("equal-c2-vector", 16000, 2, 52, 2, torch.int16, True),
    ("f32-stereo", 48000, 2, 120, 2, torch.float32, True),
    ("f32-mono", 48000, 1, 3 * 1028, 2, torch.float32, True),
    ("f32-c3", 48000, 3, 30, 2, torch.float32, False),
    ("c8", 48000, 8, 66, 2, torch.int16, False),
    ("short", 48000, 1, 30, 2, torch.int16, False),
    ("short-b3", 48000, 1, 30, 3, torch.int16, False),
]


@pytest.mark.parametrize("name,rate,channels,n_in,batch,dtype,vector", GEOMETRY, ids=[g[0] for g in GEOMETRY])
def test_equals_reference(native, name, rate, channels, n_in, batch, dtype, vector):
    from aiko_services_amd.ops import audio as A
    n_in = n_in(_tile()) if callable(n_in) else n_in
    pcm, hist, filt, L, M, ref, ref_hist = case(rate, channels, n_in, batch, dtype)
    T, n_out = filt.shape[1], n_in * L // M
    if name in ("tile+1", "2tiles+5", "tile+8"):                  # a partial last tile, and the hist_out workgroup
        assert n_out % A.RESAMPLE_TILE in (1, 5, 8) and n_out > A.RESAMPLE_TILE
        assert A.resample_grid(n_out, batch) == (n_out // A.RESAMPLE_TILE + 2, batch)
    if name == "441-phases":
        assert n_out == 1280 and L == 160
    if name == "96k":
        assert T == 192
    if name.startswith("short"):
        assert n_in < T - 1 and hist.abs().max() > 0.5
        assert torch.equal(ref_hist[:, :T - 1 - n_in], hist[:, n_in:])          # old history, shifted
    d = pcm.cuda()
    assert A.resample_uses_vector(d) == vector
    out, hist_out = run(d, hist, filt, L, M)
    assert torch.equal(out, ref) and torch.equal(hist_out, ref_hist)
    assert torch.equal(d.cpu(), pcm)
    fresh = A.resample(d, hist.cuda(), filt.cuda(), L, M)          # the default outputs: new, same values
    assert fresh[0].shape == (batch, n_out) and fresh[1].shape == (batch, T - 1)
    assert torch.equal(fresh[0].cpu(), ref) and torch.equal(fresh[1].cpu(), ref_hist)


def test_vector_and_scalar_paths_agree(native):
    from aiko_services_amd.ops import audio as A
    pcm, hist, filt, L, M, ref, ref_hist = case(48000, 2, 3 * 344)
    aligned, shifted = pcm.cuda(), misaligned(pcm)
    assert A.resample_uses_vector(aligned) and not A.resample_uses_vector(shifted)
    for d in (aligned, shifted):
        out, hist_out = run(d, hist, filt, L, M)
        assert torch.equal(out, ref) and torch.equal(hist_out, ref_hist)


@pytest.mark.parametrize("pattern", ["min", "max", "alternating"])
def test_extremes(native, pattern):
    from aiko_services_amd.ops import audio as A
    from aiko_services_amd.ops.reference import resample_ref
    filt, L, M = A.resample_filter(48000, 16000)
    n_in = 240
    pcm = torch.full((2, n_in, 2), -32768 if pattern == "min" else 32767, dtype=torch.int16)
    if pattern == "alternating":
        pcm[:, ::2] = -32768
    hist = torch.ones(2, filt.shape[1] - 1)
    hist[1] = -1.0
    ref, ref_hist = resample_ref(pcm, hist, filt, L, M)
    out, hist_out = run(pcm.cuda(), hist, filt, L, M)
    assert torch.isfinite(out).all() and torch.isfinite(hist_out).all()
    assert torch.equal(out, ref) and torch.equal(hist_out, ref_hist)
    assert ref.abs().max() >= 0.99                                # full scale (a step rings above it)


def test_streaming_with_carried_history(native):
    from aiko_services_amd.ops import audio as A
    n_in = 441 * 8
    whole = case(44100, 2, 3 * n_in, hist="zeros")
    pcm, _, filt, L, M, ref, ref_hist = whole
    T = filt.shape[1]
    f = filt.cuda()
    hists = [torch.zeros(2, T - 1, device="cuda"), torch.full((2, T - 1), float("nan"), device="cuda")]
    outs = []
    for i in range(3):
        chunk = pcm[:, i * n_in:(i + 1) * n_in].contiguous().cuda()
        out, _ = A.resample(chunk, hists[i % 2], f, L, M, hist_out=hists[(i + 1) % 2])
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(outs, dim=1).cpu(), ref) and torch.equal(hists[1].cpu(), ref_hist)


# ---- guard bands ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["441-phases", "short", "misaligned"])
def test_guard_bands(native, name):
    from aiko_services_amd.ops import audio as A
    rate, channels, n_in = {"441-phases": (44100, 2, 441 * 8), "short": (48000, 1, 30),
                            "misaligned": (48000, 2, 3 * 344)}[name]
    pcm, hist, filt, L, M, ref, ref_hist = case(rate, channels, n_in)
    B, T, n_out = 2, filt.shape[1], n_in * L // M
    plain = run(misaligned(pcm) if name == "misaligned" else pcm.cuda(), hist, filt, L, M)
    checks = []
    if name == "misaligned":                              # one int16 into the guarded interior
        flat, c = guarded((pcm.numel() + 1,), torch.int16, "cuda", name="pcm")
        gp = flat[1:].view(pcm.shape)
        gp.copy_(pcm)
        assert not A.resample_uses_vector(gp)
    else:
        gp, c = guarded(pcm.shape, torch.int16, "cuda", values=pcm, name="pcm")
        assert A.resample_uses_vector(gp) == (name == "441-phases")
    checks.append(c)
    gh, c = guarded((B, T - 1), torch.float32, "cuda", values=hist, name="hist")
    checks.append(c)
    gf, c = guarded(filt.shape, torch.float32, "cuda", values=filt, name="filt")
    checks.append(c)
    go, c = guarded((B, n_out), torch.float32, "cuda", name="out")
    checks.append(c)
    gho, c = guarded((B, T - 1), torch.float32, "cuda", name="hist_out")
    checks.append(c)
    A.resample(gp, gh, gf, L, M, out=go, hist_out=gho)
    torch.cuda.synchronize()
    for c in checks:
        c()
    assert torch.equal(gp.cpu(), pcm) and torch.equal(gh.cpu(), hist) and torch.equal(gf.cpu(), filt)
    # the outputs were all NaN and the guards still are: equal to the unguarded run (and to the
    # reference) means every element was written from values inside the operands
    assert torch.equal(go.cpu(), plain[0]) and torch.equal(gho.cpu(), plain[1])
    assert torch.equal(go.cpu(), ref) and torch.equal(gho.cpu(), ref_hist)


# ---- hipGraph -------------------------------------------------------------------------------

def test_graph_replay_follows_the_input(native):
    from aiko_services_amd.ops import audio as A
    n_in = 441 * 8
    first = case(44100, 2, n_in)
    other = case(44100, 2, n_in, seed=77)
    _, _, filt, L, M, _, _ = first
    T = filt.shape[1]
    pcm, hist, f = first[0].cuda(), first[1].cuda(), filt.cuda()
    out = torch.empty(2, n_in * L // M, device="cuda")
    hist_out = torch.empty(2, T - 1, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.resample(pcm, hist, f, L, M, out=out, hist_out=hist_out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        A.resample(pcm, hist, f, L, M, out=out, hist_out=hist_out)
    assert not torch.equal(first[5], other[5])
    for c in (first, other, first):
        pcm.copy_(c[0])
        hist.copy_(c[1])
        out.fill_(float("nan"))
        hist_out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), c[5]) and torch.equal(hist_out.cpu(), c[6])


# ---- refusals -------------------------------------------------------------------------------

def test_refusals(native):
    from aiko_services_amd.ops import audio as A
    n_in = 120
    host, hhist, filt, L, M, ref, ref_hist = case(48000, 2, n_in)
    T = filt.shape[1]
    pcm, hist, f = host.cuda(), hhist.cuda(), filt.cuda()
    out = torch.full((2, n_in // 3), 7.0, device="cuda")
    hist_out = torch.full((2, T - 1), 7.0, device="cuda")
    wide = torch.zeros(2, n_in, 4, dtype=torch.int16, device="cuda")
    assert not wide[:, :, ::2].is_contiguous()

    def call(pcm=pcm, hist=hist, filt=f, L=L, M=M, out=out, hist_out=hist_out):
        return A.resample(pcm, hist, filt, L, M, out=out, hist_out=hist_out)

    for match, kw in [
            ("n_in \\* L % M", dict(pcm=pcm[:, :100].contiguous())),               # 100 is no multiple of 3
            ("channels", dict(pcm=torch.zeros(2, n_in, 9, dtype=torch.int16, device="cuda"))),
            ("pcm int16 or fp32", dict(pcm=pcm.int())),
            ("pcm int16 or fp32", dict(pcm=pcm.view(2, n_in * 2))),
            ("contiguous", dict(pcm=wide[:, :, ::2])),
            ("hist fp32", dict(hist=torch.zeros(2, T, device="cuda"))),
            ("hist fp32", dict(hist=torch.zeros(3, T - 1, device="cuda"))),
            ("hist fp32", dict(hist=hist.double())),
            ("hist_out fp32", dict(hist_out=torch.zeros(2, T - 2, device="cuda"))),
            ("hist_out and hist overlap", dict(hist_out=hist)),
            ("out fp32", dict(out=torch.zeros(2, n_in // 3 + 1, device="cuda"))),
            ("out fp32", dict(out=torch.zeros(1, n_in // 3, device="cuda"))),
            ("out fp32", dict(out=torch.zeros(2, n_in // 3, dtype=torch.float64, device="cuda"))),
            ("filt fp32 \\[L, T\\]", dict(L=2, M=6)),                                # filt has one row
            ("filt fp32 \\[L, T\\]", dict(filt=f.view(-1))),
            ("bad ratio", dict(L=0)),
            ("GPU tensor", dict(pcm=host)),
            ("GPU tensor", dict(hist=hhist)),
            ("GPU tensor", dict(filt=filt)),
            ("GPU tensor", dict(out=torch.zeros(2, n_in // 3)))]:
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    # pcm inside hist_out's allocation
    big = torch.zeros(2 * (T - 1) + n_in * 2, device="cuda")
    with pytest.raises(RuntimeError, match="hist_out and pcm overlap"):
        call(pcm=big.view(torch.int16)[:2 * n_in * 2].view(2, n_in, 2), hist_out=big[:2 * (T - 1)].view(2, T - 1))
    with pytest.raises(ValueError, match="n_in"):                 # the wrapper, before it allocates
        A.resample(pcm[:, :100].contiguous(), hist, f, L, M)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (hist_out == 7.0).all()         # no refused call wrote anything
    got = call()
    torch.cuda.synchronize()
    assert torch.equal(got[0].cpu(), ref) and torch.equal(got[1].cpu(), ref_hist)


# ---- elements -------------------------------------------------------------------------------

SPEECH = "aiko_services_amd.elements.gpu.speech"
INGEST = "aiko_services_amd.elements.gpu.audio_ingest"
EXAMPLES = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/speech"


def _create(definition, stream_id="a"):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<audio>", parse_pipeline_definition_dict(definition), None, None, stream_id, [],
                                     0, None, 60, queue_response=q)
    return p, q


def _spy(element):
    """Clones of the ``audio`` the element is given."""
    inner, seen = element.process_frame, []

    def spy(stream, audio, *args, **kw):
        seen.append(audio.clone())
        return inner(stream, audio, *args, **kw)

    element.process_frame = spy
    return seen


def _element(name, module, inputs, outputs, parameters):
    return {"name": name, "input": [{"name": n, "type": "tensor"} for n in inputs],
            "output": [{"name": n, "type": "tensor"} for n in outputs], "parameters": parameters,
            "deploy": {"local": {"module": module}}}


def _chunks_pipeline(source, lanes):
    b, c, rate, chunk, frames = 2, 2, 48000, 0.01, 3
    n_in = int(chunk * rate)
    d = {"version": 0, "name": "p_pcm", "runtime": "python", "graph": ["(AudioChunks AudioResample)"],
         "parameters": {"gpu_lanes": lanes} if lanes else {},
         "elements": [
             _element("AudioChunks", SPEECH, ["audio_samples"] if source == "host" else [], ["audio", "t_submit"],
                      {"format": "pcm16", "sample_rate": rate, "channels": c, "streams": b, "chunk": chunk, "pool": 2,
                       "seed": 4}),
             _element("AudioResample", INGEST, ["audio"], ["audio"],
                      {"sample_rate_in": rate, "sample_rate_out": 16000, "channels": c})]}
    p, q = _create(d)
    seen = _spy(p.pipeline_graph.get_node("AudioResample").element)
    g = torch.Generator().manual_seed(11)
    outs = []
    for i in range(frames):
        data = {}
        if source == "host":                              # as a capture thread hands it over: numpy, [B, n, C]
            data = {"audio_samples": torch.randint(-32768, 32768, (b, n_in, c), generator=g).to(torch.int16).numpy()}
        p.process_frame({"stream_id": "a", "frame_id": i}, data)
        info, out = q.get_nowait()
        assert info["state"] == 0, out
        torch.cuda.synchronize()
        outs.append(out["audio"].clone())
        if source == "host":
            assert torch.equal(seen[i].cpu(), torch.from_numpy(data["audio_samples"]))
    assert all(s.dtype == torch.int16 and s.is_cuda and tuple(s.shape) == (b, n_in, c) for s in seen)
    return p, torch.cat([s.cpu() for s in seen], dim=1), torch.cat(outs, dim=1).cpu()


@pytest.mark.parametrize("source", ["host", "synthetic"])
def test_pcm16_chunks_into_resample(native, source):
    from aiko_services_amd.ops import audio as A
    from aiko_services_amd.ops.reference import resample_ref
    from aiko_services_amd.pipeline.stream import StreamEvent
    p, pcm, got = _chunks_pipeline(source, 0)
    filt, L, M = A.resample_filter(48000, 16000)
    ref, _ = resample_ref(pcm, torch.zeros(2, filt.shape[1] - 1), filt, L, M)
    assert tuple(got.shape) == (2, 3 * 160) and torch.equal(got, ref)
    assert pcm.float().abs().max() > 1000                         # a signal, not silence
    p2, pcm2, got2 = _chunks_pipeline(source, 2)                  # two frame lanes: the same samples
    assert p2.share["gpu_lanes"] == 2
    assert torch.equal(pcm2, pcm) and torch.equal(got2, got)
    el = p.pipeline_graph.get_node("AudioResample").element
    assert el.share["resample_delay"] == 0.001
    # [B, n*C] is the same chunk; a chunk that is no multiple of M = 3 samples ends the frame
    before = el._cur
    event, data = el.process_frame(None, audio=torch.zeros(2, 100, 2, dtype=torch.int16, device="cuda"))
    assert event == StreamEvent.ERROR and "multiple of 3" in data["diagnostic"] and el._cur == before
    event, data = el.process_frame(None, audio=torch.zeros(2, 481, dtype=torch.int16, device="cuda"))
    assert event == StreamEvent.ERROR and "required" in data["diagnostic"]
    event, data = el.process_frame(None, audio=torch.zeros(2, 480, 2, dtype=torch.int32, device="cuda"))
    assert event == StreamEvent.ERROR
    event, data = el.process_frame(None, audio=torch.zeros(2, 480, 2, dtype=torch.int16))          # on the host
    assert event == StreamEvent.ERROR and el._cur == before


def test_wav48k_example(native, tmp_path, monkeypatch):
    """examples/speech/pipeline_wav48k_encoder.json on a 12 s file: the generator is driven from
    here, frame by frame, to the end of the file."""
    from aiko_services_amd.elements.media.audio_io import AudioReadFile
    from aiko_services_amd.ops import audio as A
    from aiko_services_amd.ops.reference import resample_ref
    from aiko_services_amd.pipeline.stream import StreamEvent
    rate, seconds = 48000, 12
    t = np.arange(rate * seconds) / rate
    rng = np.random.default_rng(3)
    x = np.stack([0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 11000 * t),
                  0.3 * np.sin(2 * np.pi * 330 * t) + 0.02 * rng.standard_normal(len(t))], axis=1)
    pcm = np.round(x * 32767).astype(np.int16)
    path = tmp_path / "speech_48k_stereo.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    d = json.loads((EXAMPLES / "pipeline_wav48k_encoder.json").read_text())
    assert d["graph"] == ["(AudioReadFile AudioChunks AudioResample AudioWindow WhisperEncoder FeatureSink)"]
    by_name = {e["name"]: e for e in d["elements"]}
    assert by_name["AudioReadFile"]["parameters"]["raw"] is True
    assert by_name["AudioChunks"]["parameters"]["format"] == "pcm16"
    by_name["AudioReadFile"]["parameters"]["data_sources"] = f"(file://{path})"
    by_name["WhisperEncoder"]["parameters"].update(size="tiny", autotune=False)
    monkeypatch.setattr(AudioReadFile, "create_frames", lambda self, *a, **k: None)   # no generator thread
    p, q = _create(d, "w")
    reader = p.pipeline_graph.get_node("AudioReadFile").element
    seen = _spy(p.pipeline_graph.get_node("AudioWindow").element)
    stream = p.stream_leases["w"].stream
    features = []
    for i in range(10):
        event, data = reader.frame_generator(stream, i)
        if event == StreamEvent.STOP:
            break
        assert event == StreamEvent.OKAY and data["audio_samples"].shape == (5 * rate, 2)
        p.process_frame({"stream_id": "w", "frame_id": i}, data)
        info, out = q.get_nowait()
        assert info["state"] == 0, out
        features.append(out["embedding"].wait()["pooled"].clone())
    assert len(features) == 3 and event == StreamEvent.STOP       # 5 + 5 + 2 s: the end of the file
    torch.cuda.synchronize()
    filt, L, M = A.resample_filter(48000, 16000)
    padded = np.concatenate([pcm, np.zeros((3 * rate, 2), np.int16)])
    ref, _ = resample_ref(torch.from_numpy(padded)[None], torch.zeros(1, filt.shape[1] - 1), filt, L, M)
    audio = torch.cat(seen, dim=1)
    assert tuple(audio.shape) == (1, 15 * 16000) and torch.equal(audio.cpu(), ref)
    assert torch.isfinite(torch.stack(features)).all()
    # the same audio straight into AudioWindow: the same features
    d2 = dict(d, name="p_direct", graph=["(AudioWindow WhisperEncoder FeatureSink)"],
              elements=[by_name["AudioWindow"], by_name["WhisperEncoder"],
                        dict(by_name["FeatureSink"], input=[{"name": "features", "type": "tensor"}])])
    p2, q2 = _create(d2, "w2")
    for i, chunk in enumerate(seen):
        p2.process_frame({"stream_id": "w2", "frame_id": i}, {"audio": chunk})
        info, out = q2.get_nowait()
        assert info["state"] == 0, out
        assert torch.equal(out["embedding"].wait()["pooled"], features[i]), i
