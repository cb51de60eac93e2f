"""The sample-rate converter on the CPU: the filter design table, ``resample_ref`` (the definition
the kernel matches bit for bit) streamed against one shot, its downmix against ``read_wav``, what it
passes and what it stops, and ``AudioReadFile`` with ``raw: true``."""
import types
import wave

import numpy as np
import pytest
import torch

from aiko_services_amd.ops import audio as A
from aiko_services_amd.ops.reference import resample_ref

# input rate -> (L, M, T) for output at 16 kHz with the default design
DESIGN = {48000: (1, 3, 96), 44100: (160, 441, 90), 32000: (1, 2, 64), 22050: (320, 441, 46),
          96000: (1, 6, 192), 8000: (2, 1, 32), 16000: (1, 1, 1)}


def test_design_table():
    for rate, (L, M, T) in DESIGN.items():
        filt, l, m = A.resample_filter(rate, 16000)
        assert (l, m, tuple(filt.shape)) == (L, M, (L, T)), rate
        assert filt.dtype == torch.float32 and not filt.is_cuda
        assert (filt.double().sum(dim=1) - 1.0).abs().max() <= 1e-6, rate
        assert A.resample_filter(rate, 16000)[0] is filt                 # cached
        assert A.resample_lds_bytes(L, M, T) <= A.RESAMPLE_MAX_LDS
    assert A.resample_filter(16000, 16000)[0].tolist() == [[1.0]]
    assert A.resample_delay(48000, 16000) == 0.001 and A.resample_delay(16000, 16000) == 0.0
    assert A.resample_delay(44100, 16000) == 45 / 44100
    with pytest.raises(ValueError, match="taps"):                        # L*T = 640 * 32 > 16384
        A.resample_filter(11025, 16000)
    assert A.resample_filter(192000, 8000)[1:] == (1, 24)                # steep, and still served
    with pytest.raises(ValueError, match="LDS"):                         # M/L = 40: a tile's span is 165 KiB
        A.resample_filter(640000, 16000)


def _pcm(b, n, c, seed, dtype=torch.int16):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int16:
        return torch.randint(-32768, 32768, (b, n, c), generator=g).to(torch.int16)
    return torch.rand(b, n, c, generator=g) * 2 - 1


@pytest.mark.parametrize("rate,channels,n_in", [(44100, 2, 441 * 40), (48000, 1, 120), (8000, 3, 40), (16000, 2, 50)])
def test_streaming_equals_one_shot(rate, channels, n_in):
    filt, L, M = A.resample_filter(rate, 16000)
    T = filt.shape[1]
    chunks = [_pcm(2, n_in, channels, 10 * rate + i) for i in range(3)]
    zeros = torch.zeros(2, T - 1)
    whole, whole_hist = resample_ref(torch.cat(chunks, dim=1), zeros, filt, L, M)
    hist, outs = zeros, []
    for c in chunks:
        out, hist = resample_ref(c, hist, filt, L, M)
        assert tuple(out.shape) == (2, n_in * L // M) and tuple(hist.shape) == (2, T - 1)
        outs.append(out)
    assert torch.equal(torch.cat(outs, dim=1), whole) and torch.equal(hist, whole_hist)
    if T > 1:
        assert whole.abs().max() > 0.01


def test_reference_refuses_a_partial_phase():
    filt, L, M = A.resample_filter(48000, 16000)
    with pytest.raises(ValueError, match="n_in"):
        resample_ref(_pcm(1, 100, 1, 0), torch.zeros(1, 95), filt, L, M)


@pytest.mark.parametrize("channels", [1, 2])
def test_downmix_equals_read_wav(tmp_path, channels):
    from aiko_services_amd.elements.media.audio_io import read_wav
    pcm = _pcm(1, 999, channels, 5)
    pcm[0, :4] = torch.tensor([[-32768] * channels, [32767] * channels, [-32768, 32767][:channels], [1] * channels])
    path = tmp_path / "x.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.numpy().tobytes())
    want, rate = read_wav(path)
    filt, L, M = A.resample_filter(rate, 16000)
    out, hist = resample_ref(pcm, torch.zeros(1, 0), filt, L, M)
    assert tuple(hist.shape) == (1, 0) and want.dtype == np.float32
    assert np.array_equal(out[0].numpy(), want)


# ---- quality ----------------------------------------------------------------------------------

def _tone(freq, rate, n):
    t = np.arange(n, dtype=np.float64) / rate
    return np.round(0.5 * 32767.0 * np.sin(2 * np.pi * freq * t)).astype(np.int16)


def _db(x, ref):
    return 20 * np.log10(max(np.sqrt(np.mean(np.square(x))), 1e-30) / ref)


@pytest.mark.parametrize("rate", [48000, 44100])
def test_pass_and_stop_bands(rate):
    filt, L, M = A.resample_filter(rate, 16000)
    T = filt.shape[1]
    n_in = M * (24000 // M)                                              # about half a second
    skip = T                                                             # the start-up: zeros in hist
    tone_rms = 0.5 * 32767.0 / 32768.0 / np.sqrt(2.0)
    for freq in (440, 1000, 3000):
        pcm = torch.from_numpy(_tone(freq, rate, n_in))[None, :, None]
        out = resample_ref(pcm, torch.zeros(1, T - 1), filt, L, M)[0][0].double().numpy()
        t = np.arange(len(out), dtype=np.float64) / 16000.0 - A.resample_delay(rate, 16000)
        ideal = 0.5 * 32767.0 / 32768.0 * np.sin(2 * np.pi * freq * t)
        err = _db((out - ideal)[skip:], tone_rms)
        print(f"{rate} Hz, pass {freq} Hz: error {err:.1f} dB")
        assert err <= -80.0, (rate, freq, err)
    for freq in (9000, 10000, 12000, 15000, 20000):
        pcm = torch.from_numpy(_tone(freq, rate, n_in))[None, :, None]
        out = resample_ref(pcm, torch.zeros(1, T - 1), filt, L, M)[0][0].double().numpy()
        level = _db(out[skip:], tone_rms)
        print(f"{rate} Hz, stop {freq} Hz: output {level:.1f} dB")
        assert level <= -85.0, (rate, freq, level)


def test_linear_interpolation_aliases():
    """What the device path replaces: ``resample_linear`` keeps every third sample of 48 kHz audio,
    so a 10 kHz tone comes out as a 6 kHz alias at full level."""
    from aiko_services_amd.elements.media.audio_io import resample_linear
    x = _tone(10000, 48000, 24000).astype(np.float32) / 32768.0
    level = _db(resample_linear(x, 48000, 16000).astype(np.float64), 0.5 * 32767.0 / 32768.0 / np.sqrt(2.0))
    print(f"resample_linear, 10 kHz at 48 kHz: output {level:.1f} dB")
    assert level > -1.0


# ---- AudioReadFile raw: true ------------------------------------------------------------------

def _reader(parameters):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    d = {"version": 0, "name": "p_wav_raw", "runtime": "python", "graph": ["(AudioReadFile)"], "parameters": {},
         "elements": [{"name": "AudioReadFile", "input": [{"name": "audio_samples", "type": "ndarray"}],
                       "output": [{"name": "audio_samples", "type": "ndarray"}], "parameters": parameters,
                       "deploy": {"local": {"module": "aiko_services_amd.elements.media.audio_io"}}}]}
    p = PipelineImpl.create_pipeline("<wav>", parse_pipeline_definition_dict(d), None, None, None, [], 0, None, 60)
    return p.pipeline_graph.get_node("AudioReadFile").element


def _frames(reader, path):
    """Drive the element's frame generator as the engine's generator thread does."""
    stream = types.SimpleNamespace(variables={"source_paths_generator": iter([(path, None)]), "audio_chunks": None})
    out = []
    for i in range(100):
        event, data = reader.frame_generator(stream, i)
        out.append((event, data))
        if event != 0:
            break
    return out


def test_raw_wav_chunks(tmp_path):
    from aiko_services_amd.pipeline.stream import StreamEvent
    rate, n = 48000, 48000 + 4800                                        # 1.1 s: three chunks of 0.5 s
    pcm = _pcm(1, n, 2, 9)[0].numpy()
    path = tmp_path / "stereo.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    got = _frames(_reader({"raw": True, "sample_rate": rate, "chunk_duration": 0.5}), path)
    assert [e for e, _ in got] == [StreamEvent.OKAY] * 3 + [StreamEvent.STOP]
    chunks = [d["audio_samples"] for _, d in got[:3]]
    assert all(c.dtype == np.int16 and c.shape == (24000, 2) for c in chunks)
    whole = np.concatenate(chunks)
    assert np.array_equal(whole[:n], pcm) and not whole[n:].any()        # the tail is padded with zeros
    # the default is unchanged: float32 mono, resampled on the host
    got = _frames(_reader({"sample_rate": 16000, "chunk_duration": 0.5}), path)
    assert got[0][0] == StreamEvent.OKAY and got[0][1]["audio_samples"].dtype == np.float32
    assert got[0][1]["audio_samples"].shape == (8000,)
    # a file at another rate than the parameter, or not 16-bit: ERROR
    event, data = _frames(_reader({"raw": True, "sample_rate": 44100, "chunk_duration": 0.5}), path)[0]
    assert event == StreamEvent.ERROR and "48000" in data["diagnostic"]
    path8 = tmp_path / "u8.wav"
    with wave.open(str(path8), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(1)
        w.setframerate(rate)
        w.writeframes(bytes(1000))
    event, data = _frames(_reader({"raw": True, "sample_rate": rate}), path8)[0]
    assert event == StreamEvent.ERROR and "8-bit" in data["diagnostic"]
