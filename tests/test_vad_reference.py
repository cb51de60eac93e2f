"""``voice_activity_ref`` (ops/reference.py), the definition the vad kernels are held to: the level
table on hand-computed energies, chunked against one-shot processing, what the defaults do on a
scripted room, the state's edge cases and the parameter refusals.  CPU only."""
import math

import pytest
import torch

import vad_scenes as S

RATE = 16000


def _ref(audio, state=None, **kw):
    from aiko_services_amd.ops.reference import voice_activity_ref
    from aiko_services_amd.ops.vad import new_state
    audio = audio if audio.dim() == 2 else audio[None]
    return voice_activity_ref(audio.contiguous(), state or new_state(audio.shape[0], "cpu"), **kw)


def _equal(got, want, where):
    names = ("mask", "seg", "count", "speech", "silent", "level", "zc")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), f"{where}: {name}"
    assert torch.equal(got[7].v, want[7].v), f"{where}: state"


def test_scenes_cover_what_they_claim():
    S.assert_conditions()


def test_level_table():
    """E = 0, 1, 15, 16, 2^32, 480 * 2^30 by hand: p = -, 0, 3, 4, 32, 38 (480 = 0b111100000, 9 bits);
    mant = -, 0, (15 << 1) & 15 = 14, 0, 0, 0b11110 & 15 = 14."""
    from aiko_services_amd.ops.reference import vad_level_ref
    want = {0: 0, 1: 16, 15: 16 * 4 + 14, 16: 16 * 5, 2 ** 32: 16 * 33, 480 * 2 ** 30: 16 * 39 + 14}
    assert {E: vad_level_ref(E) for E in want} == want
    # the same energies from samples: frames of 480, one stream each
    u = 1.0 / 32768.0
    rows = torch.zeros(6, 480)
    rows[1, 7] = u                                          # E = 1
    rows[2, :15] = -u                                       # E = 15
    rows[3, 479] = 4 * u                                    # E = 16
    rows[4, 100:104] = -1.0                                 # E = 4 * 2^30
    rows[5, :] = -1.0                                       # E = 480 * 2^30: past 32 bits
    out = _ref(rows, frame=480)
    assert out[5][:, 0].tolist() == list(want.values())
    assert out[6][:, 0].tolist() == [0, 0, 1, 0, 2, 0]      # -1 -> 0 is a sign change of q, 0 -> 1 is none


def test_full_scale_sine_is_612():
    t = torch.arange(320, dtype=torch.float64) / RATE
    out = _ref(torch.sin(2 * math.pi * 440.0 * t).float())
    assert int(out[5][0, 0]) == 612 and int(out[6][0, 0]) == 17      # 8.8 periods: 17 sign changes


def test_sample_rule():
    """NaN -> 0, +-inf and +-4 clamp, -1e-6 -> 0 (not negative), (k + 0.5) / 32768 half to even."""
    x = torch.zeros(1, 160)
    x[0, :10] = torch.tensor([float("nan"), float("inf"), -float("inf"), 4.0, -4.0, -1e-6, 2.5 / 32768, 3.5 / 32768,
                              -2.5 / 32768, 1e-40])
    E = 32767 ** 2 * 2 + 32768 ** 2 * 2 + 2 ** 2 + 4 ** 2 + 2 ** 2
    from aiko_services_amd.ops.reference import vad_level_ref
    out = _ref(x, frame=160)
    assert int(out[5][0, 0]) == vad_level_ref(E)
    # signs of q: 0 + - + - 0 + + - 0 0...: changes at 2, 3, 4, 5, 8, 9
    assert int(out[6][0, 0]) == 6


@pytest.mark.parametrize("name,frame", [("bursts", 160), ("sharp", S.SHARP_FRAME)])
def test_chunked_equals_one_shot_at_every_cut(name, frame):
    s = S.scene(name, frame)
    F = s.audio.shape[1] // frame
    whole = _ref(s.audio, s.state0, **s.kw)
    assert torch.equal(whole[0], S.whole_mask(name, frame))        # ... and the scene's own chunks
    for cut in range(1, F):
        a = _ref(s.audio[:, :cut * frame], s.state0, **s.kw)
        b = _ref(s.audio[:, cut * frame:], a[7], **s.kw)
        for i in (0, 5, 6):                                 # mask, level, zc
            assert torch.equal(torch.cat([a[i], b[i]], dim=1), whole[i]), (cut, i)
        assert torch.equal(a[3] + b[3], whole[3]) and torch.equal(b[4], whole[4]), cut
        assert torch.equal(b[7].v, whole[7].v), cut


def _room(seconds=12.0, seed=0):
    """Noise at 0.02, a 0.3 tone at 2..3.5 s, a 40 ms blip at 6 s, a 0.05 tone at 8..9 s, the noise
    12 dB up from 10 s."""
    g = torch.Generator().manual_seed(seed)
    n = int(seconds * RATE)
    t = torch.arange(n, dtype=torch.float64) / RATE
    x = 0.02 * torch.randn(n, generator=g)
    x[10 * RATE:] *= 10 ** (12 / 20)
    for a, b, amp in ((2.0, 3.5, 0.3), (6.0, 6.04, 0.3), (8.0, 9.0, 0.05)):
        i0, i1 = int(a * RATE), int(b * RATE)
        x[i0:i1] += (amp * torch.sin(2 * math.pi * 440.0 * t[i0:i1])).float()
    return x


@pytest.mark.parametrize("frame", S.FRAMES)
def test_defaults_on_a_room(frame):
    x = _room()
    out = _ref(x, frame=frame)
    sec = frame / RATE
    segs = [(a * sec, b * sec) for a, b in out[1][0, :int(out[2][0])].tolist()]
    tone = [s for s in segs if s[0] < 5]
    assert len(tone) == 1 and 2.0 <= tone[0][0] <= 2.0 + 3 * sec        # onset lags by attack - 1 frames
    assert 3.5 + 15 * sec <= tone[0][1] <= 3.5 + 17 * sec               # the hangover is part of the speech
    assert not [s for s in segs if 7.5 < s[0] < 9.5]                    # the 0.05 tone is ignored
    blip = [s for s in segs if 5.5 < s[0] < 7]
    if frame == 160:                                                    # four 10 ms frames meet attack 3
        assert len(blip) == 1 and abs(blip[0][0] - 6.02) < 1e-9 and abs(blip[0][1] - 6.19) < 1e-9
    else:
        assert not blip
    # the noise step reads as speech: one segment from the step on, for seconds
    step = [s for s in segs if s[0] >= 9.5]
    assert len(step) == 1 and step[0][0] <= 10.0 + 4 * sec and step[0][1] >= 11.85
    if frame != 480:
        assert step[0][1] == 12.0 and int(out[0][0, -1]) == 1          # still open when the scene ends
    # six chunks give the same mask as one call
    F = x.shape[0] // frame
    state, masks = None, []
    for i in range(6):
        a, b = i * F // 6, (i + 1) * F // 6
        step_out = _ref(x[a * frame:b * frame], state, frame=frame)
        state = step_out[7]
        masks.append(step_out[0])
    assert torch.equal(torch.cat(masks, dim=1), out[0])


def test_noise_step_is_absorbed_slowly():
    """12 dB are 4 octaves of power, 64 level units, against a threshold of 48: at speech_shift 10 the
    floor must close a quarter of the gap, ln(4/3) * 1024 = 295 frames of 20 ms, then the hangover."""
    out = _ref(_room(20.0), frame=320)
    segs = out[1][0, :int(out[2][0])].tolist()
    a, b = segs[-1]
    assert a * 0.02 <= 10.1 and 10.0 + 0.02 * 250 <= b * 0.02 <= 10.0 + 0.02 * 360
    assert int(out[0][0, b:].sum()) == 0 and int(out[4][0]) == 0


def test_seen_saturates_and_empty_state_rules():
    from aiko_services_amd.ops.vad import VadState
    s = S.scene("bursts", 160)
    chunk = s.chunks()[0]
    top = 2 ** 31 - 1
    v = torch.zeros(S.B, 8, dtype=torch.int32)
    v[:, 1] = torch.tensor([top - 3, top, top - 9])
    out = _ref(chunk, VadState(v), **s.kw)
    assert out[7].v[:, 1].tolist() == [top, top, top]       # 9 frames
    # seen <= 0: the empty state whatever the other columns hold
    empty = _ref(chunk, **s.kw)
    g = torch.Generator().manual_seed(3)
    for seen in (0, -1, -2 ** 31):
        v = torch.randint(-2 ** 31, 2 ** 31 - 1, (S.B, 8), generator=g).to(torch.int32)
        v[:, 1] = seen
        v[0, 4], v[1, 4] = 1, -1                            # on set: would hold a run open
        _equal(_ref(chunk, VadState(v), **s.kw), empty, f"seen {seen}")
    # since starts at 2^30 and stays there until speech (stream 1's first burst is in this chunk)
    assert empty[4].tolist() == [1, 0, 1] and empty[7].v[:, 5].tolist() == [2 ** 30, 0, 2 ** 30]


def test_parameter_refusals():
    from aiko_services_amd.ops.vad import check_parameters
    check_parameters()
    check_parameters(frame=480, threshold=1023, min_level=1023, up_shift=16, speech_shift=0, down_shift=16,
                     warmup=2 ** 31 - 1, attack=1, hang=0, max_zc=0, window=1, max_seg=64)
    bad = dict(frame=(0, 100, 640, True), threshold=(-1, 1024, 1.5), min_level=(-1, 1024), up_shift=(-1, 17),
               speech_shift=(-1, 17), down_shift=(-1, 17), warmup=(0, 2 ** 31), attack=(0,), hang=(-1,),
               max_zc=(-1, 480), window=(0,), max_seg=(0, 65, True))
    for name, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=name):
                check_parameters(**{name: v})
    x = torch.zeros(1, 320)
    with pytest.raises(ValueError, match="max_seg"):
        _ref(x, max_seg=65)
    with pytest.raises(ValueError, match="whole frames"):
        _ref(torch.zeros(1, 321))
    with pytest.raises(ValueError, match="whole frames"):
        _ref(torch.zeros(1, 160 * 4097), frame=160)
    with pytest.raises(ValueError, match="fp32"):
        _ref(x.double())
