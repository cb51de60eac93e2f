"""The voice-activity kernels (``ops.vad.voice_activity``, vad_ops.hip) against the CPU reference, bit
for bit and chunk by chunk, on the scenes of vad_scenes.py; the sample rule's edge cases; the limits
of the launch; then the element in the example pipeline against direct calls, and the decoder's gate."""
import json
import queue
from pathlib import Path

import pytest
import torch

import vad_scenes as S
from kernel_guard import guarded

pytestmark = pytest.mark.gpu

NAMES = ("mask", "seg", "count", "speech", "silent", "level", "zc", "state")
B = S.B


def _flat(step):
    return [t.cpu() for t in (*step[:7], step[7].v)]


def _assert_step(got, want, where):
    for name, g, w in zip(NAMES, _flat(got), _flat(want)):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), f"{where}: {name}\n{g}\n{w}"


def _cuda_state(state):
    from aiko_services_amd.ops.vad import VadState
    return VadState(state.v.cuda())


def _place(audio, offset):
    """``audio`` on the device, contiguous, ``offset`` floats past a 16-byte boundary."""
    from aiko_services_amd.ops.vad import vad_uses_vector
    flat = torch.empty(audio.numel() + 4, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + audio.numel()].view(audio.shape)
    view.copy_(audio)
    assert view.is_contiguous() and vad_uses_vector(view) == (offset == 0)
    return view


def _ref(audio, state=None, **kw):
    from aiko_services_amd.ops.reference import voice_activity_ref
    from aiko_services_amd.ops.vad import new_state
    return voice_activity_ref(audio, state or new_state(audio.shape[0], "cpu"), **kw)


def _both(audio, where, offsets=(0, 1), state=None, **kw):
    """The kernels on ``audio`` (aligned: the float4 pass; one float off: the scalar pass) against the
    reference; returns the reference's step."""
    from aiko_services_amd.ops.vad import new_state, voice_activity
    want = _ref(audio, state, **kw)
    for offset in offsets:
        dev_state = _cuda_state(state) if state is not None else new_state(audio.shape[0], "cuda")
        got = voice_activity(_place(audio, offset), dev_state, **kw)
        torch.cuda.synchronize()
        _assert_step(got, want, f"{where}, offset {offset}")
    return want


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name,frame", S.SCENES)
def test_every_chunk_equals_reference(native, name, frame, offset):
    from aiko_services_amd.ops.vad import FRAME_TILE, frame_grid, voice_activity
    scene, want = S.scene(name, frame), S.reference(name, frame)
    state = _cuda_state(scene.state0)
    partial = 0
    for t, chunk in enumerate(scene.chunks()):
        F = chunk.shape[1] // frame
        partial += frame_grid(F, B)[0] * FRAME_TILE > F
        got = voice_activity(_place(chunk, offset), state, **scene.kw)
        torch.cuda.synchronize()
        _assert_step(got, want[t], f"{name}, frame {frame}, offset {offset}, chunk {t}")
        state = got[7]
    assert partial or name == "sharp"                       # 9 and 11 frames: a partial last tile


def _sample_rows(frame):
    """One stream per case, two frames each (the second: the first's negation, so that a count that
    ran over the frame boundary would show), and the zero crossings each first frame must give."""
    u = 1.0 / 32768.0
    rows, zc = [], []

    def case(first, z):
        rows.append(torch.cat([first, -first]))
        zc.append(z)

    x = torch.zeros(frame)
    x[:6] = torch.tensor([float("nan"), float("inf"), -float("inf"), 4.0, -4.0, float("nan")])
    case(x, 4)                                              # q: 0 32767 -32768 32767 -32768 0
    case(torch.full((frame,), -1e-6), 0)                    # q = 0 is not negative
    k = torch.arange(frame, dtype=torch.float32) - frame // 2
    case((k + 0.5) * u, 1)                                  # halves, even and odd k, both signs: -0.5 -> 0
    case(torch.full((frame,), 1e-40), 0)                    # a subnormal
    case(torch.full((frame,), -1.0), 0)                     # frame 480: E = 480 * 2^30
    alt = torch.ones(frame)
    alt[1::2] = -1.0
    case(0.25 * alt, frame - 1)
    # sign changes only at a float4 boundary (4), at the scalar pass boundary (64), at lane 63 | pass 1
    # of the float4 pass (256) and at 448, where they exist
    edges = [e for e in (4, 64, 256, 448) if e < frame]
    sign = torch.ones(frame)
    for e in edges:
        sign[e:] *= -1.0
    case(0.1 * sign, len(edges))
    return torch.stack(rows).contiguous(), zc


@pytest.mark.parametrize("frame", S.FRAMES)
def test_sample_and_frame_rule(native, frame):
    rows, zc = _sample_rows(frame)
    want = _both(rows, f"samples, frame {frame}", frame=frame)
    assert want[6][:, 0].tolist() == zc and want[6][:, 1].tolist() == zc
    same = [r for r in range(rows.shape[0]) if r != 4]      # -x has the energy of x, but for the clamp at +1.0
    assert torch.equal(want[5][same, 0], want[5][same, 1])
    if frame == 480:
        assert int(want[5][4, 0]) == 16 * 39 + 14           # 480 * 2^30 needs the 64-bit sum
    assert int(want[5][1, 0]) == 0 and int(want[5][3, 0]) == 0


def test_single_frame_and_partial_tile(native):
    from aiko_services_amd.ops.vad import FRAME_TILE, frame_grid
    s = S.scene("bursts", 320)
    for F in (1, FRAME_TILE + 2):
        assert F == 1 or (F % FRAME_TILE and frame_grid(F, B)[0] * FRAME_TILE > F > FRAME_TILE)
        _both(s.audio[:, 16 * 320:(16 + F) * 320].contiguous(), f"F = {F}", **{**s.kw, "warmup": 1, "attack": 1})


def test_the_longest_chunk(native):
    """F = 4096 at B = 1: every ballot word of the stream pass, the LDS rows full."""
    from aiko_services_amd.ops.vad import MAX_FRAMES
    g = torch.Generator().manual_seed(4096)
    script = (torch.rand(MAX_FRAMES, generator=g) < 0.3).int().tolist()
    script[0], script[-3:] = 0, [1, 1, 1]
    audio = S.script_audio([script], 160, 4096)
    want = _both(audio, "F = 4096", offsets=(0,), frame=160, warmup=1, attack=1, hang=0, max_seg=64, window=2)
    assert want[0][0].tolist() == script and int(want[2][0]) == 64 and int(want[0][0, -1]) == 1
    assert len(S.runs_of(script)) > 64 and want[1][0].tolist() == [list(r) for r in S.runs_of(script)[:64]]


def test_device_side_state_under_graph_replay(native):
    """Two chunks in one graph, ping-ponging two states: a -> b -> a."""
    from aiko_services_amd.ops.vad import new_state, voice_activity
    frame, F = 320, 20
    scene = S.scene("bursts", frame)
    kw = scene.kw
    pieces = [scene.audio[:, t * F * frame:(t + 1) * F * frame].contiguous() for t in range(6)]
    want, state = [], scene.state0
    for piece in pieces:
        want.append(_ref(piece, state, **kw))
        state = want[-1][7]
    assert any(int(w[7].v[0, 4]) for w in want) and sum(int(w[3].sum()) for w in want) > 0
    chunks = [torch.empty_like(pieces[0], device="cuda") for _ in range(2)]
    states = [new_state(B, "cuda") for _ in range(2)]
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="cuda")  # noqa: E731
    outs = [dict(mask=torch.empty(B, F, dtype=torch.uint8, device="cuda"), seg=i32(B, kw["max_seg"], 2), count=i32(B),
                 speech=i32(B), silent=i32(B), level=i32(B, F), zc=i32(B, F)) for _ in range(2)]

    def pair():
        for i in range(2):
            voice_activity(chunks[i], states[i], state_out=states[1 - i], **outs[i], **kw)

    for c, src in zip(chunks, pieces):
        c.copy_(src)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair()
    states[0].v.copy_(scene.state0.v)
    for t in range(0, 6, 2):
        for i in range(2):
            chunks[i].copy_(pieces[t + i])
            for x in (*outs[i].values(), states[1].v):      # poison: every element must be rewritten
                x.view(torch.uint8).fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        step = lambda o, s: (*(o[k] for k in NAMES[:7]), s)  # noqa: E731
        # the first step's state_out was read and then left alone: it is still chunk t's
        _assert_step(step(outs[0], states[1]), want[t], f"replay, chunk {t}")
        _assert_step(step(outs[1], states[0]), want[t + 1], f"replay, chunk {t + 1}")


@pytest.mark.parametrize("name,frame,at", [("bursts", 480, 2), ("sharp", S.SHARP_FRAME, 0)])
def test_guard_bands_and_no_poison_left(native, name, frame, at):
    from aiko_services_amd.ops.vad import VadState, voice_activity
    scene, want = S.scene(name, frame), S.reference(name, frame)
    kw = scene.kw
    chunk = scene.chunks()[at]
    before = want[at - 1][7] if at else scene.state0
    F = chunk.shape[1] // frame
    checks = []

    def g(shape, dtype, values=None, name=""):
        view, check = guarded(shape, dtype, "cuda", values=values, name=name)
        checks.append(check)
        return view

    ga = g(chunk.shape, torch.float32, chunk, "audio")
    gin = VadState(g((B, 8), torch.int32, before.v, "state"))
    gout = VadState(g((B, 8), torch.int32, name="state_out"))
    outs = dict(mask=g((B, F), torch.uint8, name="mask"), seg=g((B, kw["max_seg"], 2), torch.int32, name="seg"),
                count=g((B,), torch.int32, name="count"), speech=g((B,), torch.int32, name="speech"),
                silent=g((B,), torch.int32, name="silent"), level=g((B, F), torch.int32, name="level"),
                zc=g((B, F), torch.int32, name="zc"))
    got = voice_activity(ga, gin, state_out=gout, **outs, **kw)
    torch.cuda.synchronize()
    for check in checks:
        check()
    _assert_step(got, want[at], "guarded")
    fresh = voice_activity(chunk.cuda(), _cuda_state(before), **kw)
    torch.cuda.synchronize()
    _assert_step(got, fresh, "guarded against fresh tensors")
    # no element of any output kept its poison (0xA5 bytes): rows past count and state_out included
    for x in (outs["seg"], outs["count"], outs["speech"], outs["silent"], outs["level"], outs["zc"], gout.v):
        assert not (x.contiguous().view(torch.uint8).view(-1, 4) == 0xA5).all(1).any()
    assert int(outs["mask"].max()) <= 1
    assert all(not outs["seg"][b, int(outs["count"][b]):].any() for b in range(B))
    # the inputs are only read
    assert torch.equal(gin.v.cpu(), before.v) and torch.equal(ga.cpu(), chunk)


def test_refusals(native):
    from aiko_services_amd.ops.vad import VadState, new_state, voice_activity
    audio = torch.zeros(B, 4 * 320, device="cuda")
    state = new_state(B, "cuda")

    def refuse(match, audio=audio, state=state, error=RuntimeError, **kw):
        with pytest.raises(error, match=match):
            voice_activity(audio, state, **kw)

    refuse("n % frame", audio=torch.zeros(B, 4 * 320 + 160, device="cuda"))
    refuse("n % frame", audio=torch.zeros(B, 0, device="cuda"))
    refuse("F = 4097", audio=torch.zeros(1, 4097 * 160, device="cuda"), state=new_state(1, "cuda"), frame=160)
    refuse("audio fp32", audio=audio.half())
    refuse("audio fp32", audio=torch.zeros(B, 8 * 320, device="cuda")[:, ::2])
    refuse("state_out and state overlap", state_out=state)
    shared = torch.zeros(2 * B, dtype=torch.int32, device="cuda")
    refuse("speech and count overlap", count=shared[:B], speech=shared[B - 1:2 * B - 1])
    refuse("state int32", state=VadState(state.v.long()))
    refuse("state int32", state=new_state(B + 1, "cuda"))
    refuse("state_out int32", state_out=VadState(torch.zeros(B, 6, dtype=torch.int32, device="cuda")))
    refuse("mask uint8", mask=torch.empty(B, 5, dtype=torch.uint8, device="cuda"))
    refuse("level and zc int32", level=torch.empty(B, 4, dtype=torch.int64, device="cuda"))
    refuse("GPU tensor", state=new_state(B, "cpu"))
    # values: Python errors
    refuse("max_seg", error=ValueError, max_seg=65)
    refuse("max_seg", error=ValueError, max_seg=16, seg=torch.empty(B, 8, 2, dtype=torch.int32, device="cuda"))
    refuse("frame", error=ValueError, frame=240)
    refuse("threshold", error=ValueError, threshold=1024)
    refuse("attack", error=ValueError, attack=0)
    # the operator's own bounds, past the Python layer
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="cuda")  # noqa: E731

    def op(frame=320, threshold=48, max_zc=479, max_seg=16):
        torch.ops.aiko.voice_activity_out(audio, state.v, frame, threshold, 0, 6, 10, 1, 10, 3, 15, max_zc, 1500,
                                          i32(B, 8), i32(B, 4), i32(B, 4),
                                          torch.empty(B, 4, dtype=torch.uint8, device="cuda"), i32(B, max_seg, 2),
                                          i32(B), i32(B), i32(B))

    with pytest.raises(RuntimeError, match="1 <= max_seg <= 64"):
        op(max_seg=65)
    with pytest.raises(RuntimeError, match="threshold"):
        op(threshold=1024)
    with pytest.raises(RuntimeError, match="max_zc"):
        op(max_zc=480)
    with pytest.raises(RuntimeError, match="frame in"):
        op(frame=640)
    # inside them: the extremes of every parameter
    op()
    voice_activity(audio, state, frame=160, threshold=0, min_level=1023, up_shift=0, speech_shift=16, down_shift=0,
                   warmup=2 ** 31 - 1, attack=2 ** 31 - 1, hang=2 ** 31 - 1, max_zc=0, window=2 ** 31 - 1, max_seg=64)
    out = voice_activity(audio, state, frame=320, threshold=1023, up_shift=16, down_shift=16, warmup=1, attack=1,
                         hang=0, window=1, max_seg=1)
    torch.cuda.synchronize()
    assert out[4].tolist() == [1] * B and out[7].v[:, 1].tolist() == [4] * B


# ---- the example pipeline -------------------------------------------------------------------

EXAMPLE = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/speech/pipeline_vad_transcribe.json"
PIPE_B, PIPE_CHUNKS = 2, 4
PIPE_KW = dict(frame=320, threshold=48, min_level=0, up_shift=6, speech_shift=10, down_shift=1, warmup=4, attack=3,
               hang=5, max_zc=479, max_seg=4)
PIPE_WINDOW_S = 0.5                                        # 25 frames of 20 ms


def _definition(lanes):
    d = json.loads(EXAMPLE.read_text())
    assert d["graph"] == ["(AudioChunks AudioResample VoiceActivity AudioWindow WhisperEncoder WhisperTranscribe)"]
    d["parameters"]["gpu_lanes"] = lanes
    by_name = {e["name"]: e for e in d["elements"]}
    by_name["AudioChunks"]["input"] = [{"name": "audio_samples", "type": "ndarray"}]
    by_name["VoiceActivity"]["parameters"].update(PIPE_KW, window=PIPE_WINDOW_S)
    by_name["AudioWindow"]["parameters"].update(window=2.0)
    by_name["WhisperEncoder"]["parameters"].update(size="tiny", graph=False)
    by_name["WhisperTranscribe"]["parameters"].update(size="tiny", max_tokens=6)
    # ... and the host sink behind it
    d["graph"] = [d["graph"][0][:-1] + " VoiceResults)"]
    tensor = lambda name: {"name": name, "type": "tensor"}  # noqa: E731
    d["elements"].append({"name": "VoiceResults",
                          "input": [tensor("voice_mask"), tensor("voice_segments"), tensor("voice_counts"),
                                    tensor("voice_speech"), tensor("silent")],
                          "output": [{"name": "voice", "type": "result"}], "parameters": {},
                          "deploy": {"local": {"module": "aiko_services_amd.elements.gpu.vad"}}})
    return d


def _pcm_chunks():
    """Four 1 s chunks of 48 kHz stereo int16 for two streams: stream 0 speaks in chunks 0 and 1 (a
    burst over the cut), stream 1 in chunk 2 only."""
    scripts = [S._script(200, (20, 80)), S._script(200, (110, 130))]
    audio = S.script_audio(scripts, 960, 48)                 # a 20 ms frame is 960 samples at 48 kHz
    pcm = torch.round(audio * 32767.0).clamp(-32768, 32767).to(torch.int16)
    stereo = torch.stack([pcm, pcm], dim=2)                  # [B, n, 2]
    return [stereo[:, t * 48000:(t + 1) * 48000].contiguous().numpy() for t in range(PIPE_CHUNKS)]


def _run_pipeline(lanes):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<vad>", parse_pipeline_definition_dict(_definition(lanes)), None, None, "c", [],
                                     0, None, 60, queue_response=q)
    p.response_swag = True                     # the whole swag comes back, device tensors included
    element = p.pipeline_graph.get_node("VoiceActivity").element
    inner, seen = element.process_frame, []

    def spy(stream, audio, *args, **kw):
        seen.append(audio.clone())
        return inner(stream, audio, *args, **kw)

    element.process_frame = spy
    outs = []
    for i, chunk in enumerate(_pcm_chunks()):
        p.process_frame({"stream_id": "c", "frame_id": i}, {"audio_samples": chunk})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        torch.cuda.synchronize()               # buffers are reused per lane: copy before the next frame
        host = swag["voice"].wait()
        assert all(t.is_pinned() for t in host.values())
        for key, name in (("mask", "voice_mask"), ("seg", "voice_segments"), ("count", "voice_counts"),
                          ("speech", "voice_speech"), ("silent", "silent")):
            assert host[key].device.type == "cpu" and torch.equal(host[key], swag[name].cpu()), key
        outs.append({"source": seen[i], "mask": swag["voice_mask"].clone(), "seg": swag["voice_segments"].clone(),
                     "count": swag["voice_counts"].clone(), "speech": swag["voice_speech"].clone(),
                     "silent": swag["silent"].clone(), "tokens": swag["tokens"].clone(), "text": swag["text"]})
    assert p.share["gpu_lanes"] == lanes and len(seen) == PIPE_CHUNKS
    element.process_frame = inner
    return outs, p


def test_vad_pipeline_matches_direct_calls(native):
    from aiko_services_amd.ops.vad import new_state, voice_activity
    from aiko_services_amd.pipeline.stream import StreamEvent
    one, p = _run_pipeline(1)
    kw = dict(PIPE_KW, window=25)
    state, ref_state = new_state(PIPE_B, "cuda"), None
    eot = p.pipeline_graph.get_node("WhisperTranscribe").element.model.eot
    n_prompt = len(p.pipeline_graph.get_node("WhisperTranscribe").element.model.prompt)
    silents = []
    for i, o in enumerate(one):
        assert o["source"].shape == (PIPE_B, 16000) and o["source"].dtype == torch.float32
        got = voice_activity(o["source"], state, **kw)
        want = _ref(o["source"].cpu(), ref_state, **kw)
        state, ref_state = got[7], want[7]
        torch.cuda.synchronize()
        _assert_step(got, want, f"direct, chunk {i}")
        for key, t in zip(("mask", "seg", "count", "speech", "silent"), got):
            assert torch.equal(o[key], t), (i, key)
        silents.append(want[4].tolist())
        # the gate: a silent stream's tokens are the prompt, then end-of-text, its text "<silence>"
        for b in range(PIPE_B):
            if silents[-1][b]:
                assert (o["tokens"][b, n_prompt:] == eot).all() and o["text"][b] == "<silence>", (i, b)
    # the reference itself reports speech where the script has it, and both values of silent
    assert silents == [[0, 1], [0, 1], [1, 0], [1, 1]], silents
    two, _ = _run_pipeline(2)
    for a, b in zip(one, two):
        for key in ("source", "mask", "seg", "count", "speech", "silent", "tokens"):
            assert torch.equal(a[key], b[key]), key
    # diagnostics, and a change of the chunk length carries the state over
    element = p.pipeline_graph.get_node("VoiceActivity").element
    event, out = element.process_frame(None, torch.zeros(PIPE_B, 10 * 320, device="cuda"))
    torch.cuda.synchronize()
    assert event == StreamEvent.OKAY and out["voice_mask"].shape == (PIPE_B, 10)
    assert int(element._ring[element._cur][0].v[0, 1]) == 4 * 50 + 10
    for bad, text in ((torch.zeros(PIPE_B, 321, device="cuda"), "whole frames"),
                      (torch.zeros(PIPE_B, 320, device="cuda").half(), "audio fp32"), (None, "audio fp32"),
                      (torch.zeros(PIPE_B, 320), "audio fp32")):
        event, out = element.process_frame(None, bad)
        assert event == StreamEvent.ERROR and text in out["diagnostic"], out


# ---- the decoder's gate ---------------------------------------------------------------------

def test_silent_streams_are_done_before_the_first_step(native):
    from aiko_services_amd.models.whisper_decoder import WhisperDecoder
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(4, 301, 384, generator=g).to("cuda", torch.bfloat16)[:, :300]
    dec = WhisperDecoder("tiny", device=torch.device("cuda"))
    n_prompt = len(dec.prompt)
    plain = dec.transcribe(feats, max_new_tokens=24, check_every=0).clone()
    silent = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device="cuda")
    gated = dec.transcribe(feats, max_new_tokens=24, check_every=0, silent=silent).clone()
    assert gated.shape == plain.shape == (4, n_prompt + 24)
    for b in (1, 3):
        assert gated[b, :n_prompt].tolist() == list(dec.prompt) and (gated[b, n_prompt:] == dec.eot).all()
    for b in (0, 2):
        assert torch.equal(gated[b], plain[b]), b
    assert (plain[:, n_prompt] != dec.eot).any()            # the ungated run does decode something
    again = dec.transcribe(feats, max_new_tokens=24, check_every=0).clone()
    assert torch.equal(again, plain)                        # the gate leaves nothing behind
    # all four silent: over at the first stop_early check
    first = next(s for s in range(n_prompt, 64) if (s + 1) % 8 == 0)
    out = dec.transcribe(feats, max_new_tokens=24, check_every=8, silent=torch.ones(4, dtype=torch.int32))
    assert out.shape == (4, first + 2) and (out[:, n_prompt:] == dec.eot).all()
    with pytest.raises(ValueError, match="silent"):
        dec.transcribe(feats, max_new_tokens=4, silent=torch.zeros(3, dtype=torch.int32))
