"""Scenes of the voice-activity tests (``ops/vad.py``), shared by test_vad_reference.py (what
``voice_activity_ref`` must give, and what the scenes must cover) and test_gpu_vad.py (the kernels
against ``voice_activity_ref``, chunk by chunk).  A scene's reference run is computed once per process
and handed out unchanged.

Three streams, scripted frame by frame as quiet (noise at 0.01) or loud (a 0.3 tone of 440 Hz on top):
nine to ten octaves of power apart, against a threshold of three, so the script decides ``raw`` and
the reference's mask can be checked against it.

* ``bursts`` at every frame size: attack 3, hang 5, 120 frames cut into chunks of 9, 11, 16, 64 and 20
  (no chunk longer than 64 frames), so that one cut falls inside an attack run and one inside a
  hangover; stream 2 starts from a garbage state with ``seen < 0``.
* ``sharp``: attack 1, hang 0, so the mask is the script; ``max_seg`` 2.  Its first chunk is 96 frames,
  past the one ballot word of 64 frames that the stream pass works in: mask edges at frames 63 | 64
  and 64 | 65, a run across the word boundary, more runs than ``max_seg``, a run that ends the chunk.
  Its second chunk of 16 frames: a mask of all ones that continues that run, a mask of all zeros, and
  a run carried in that ends inside the chunk.

A plain module (no fixtures, no device requirement), like kernel_guard.py."""
from __future__ import annotations

import functools
import math

import torch

B = 3
RATE = 16000
FRAMES = (160, 320, 480)
QUIET, LOUD, TONE = 0.01, 0.3, 440.0
BURSTS_KW = dict(warmup=4, attack=3, hang=5, max_seg=4, window=30)
SHARP_KW = dict(warmup=1, attack=1, hang=0, max_seg=2, window=8)
SHARP_FRAME = 160


def script_audio(scripts, frame, seed):
    """fp32 ``[len(scripts), n]``: frame ``f`` of row ``b`` is noise, plus the tone where ``scripts[b][f]``."""
    g = torch.Generator().manual_seed(seed)
    F = len(scripts[0])
    assert all(len(s) == F for s in scripts)
    n = F * frame
    t = torch.arange(n, dtype=torch.float64) / RATE
    tone = (LOUD * torch.sin(2 * math.pi * TONE * t)).float()
    out = QUIET * torch.randn(len(scripts), n, generator=g)
    for b, s in enumerate(scripts):
        gate = torch.tensor(s, dtype=torch.float32).repeat_interleave(frame)
        out[b] += gate * tone
    return out.contiguous()


def _script(F, *loud):
    """``F`` frames, loud in the half-open ranges ``loud``."""
    s = [0] * F
    for a, b in loud:
        s[a:b] = [1] * (b - a)
    return s


class Scene:
    """``audio`` fp32 ``[B, n]`` taken in chunks of ``cuts`` frames from ``state0`` with ``kw``;
    ``scripts[b][f]`` says whether frame ``f`` of stream ``b`` is loud."""

    def __init__(self, name, frame):
        from aiko_services_amd.ops.vad import VadState, new_state
        self.name, self.frame = name, frame
        state = new_state(B, "cpu")
        if name == "bursts":
            self.kw = {**BURSTS_KW, "frame": frame}
            self.cuts = (9, 11, 16, 64, 20)
            self.scripts = [_script(120, (8, 18), (40, 42), (60, 75), (110, 120)),
                            _script(120, (5, 8), (12, 14), (34, 37), (50, 100)),
                            _script(120, (20, 36), (99, 104))]
            g = torch.Generator().manual_seed(7)
            state.v[2] = torch.randint(-2 ** 31, 2 ** 31 - 1, (8,), generator=g).to(torch.int32)
            state.v[2, 1] = -3                              # garbage, and a negative frame count
        elif name == "sharp":
            self.kw = {**SHARP_KW, "frame": frame}
            self.cuts = (96, 16)
            many = [(a, a + 1) for a in range(2, 30, 3)]    # ten runs of one frame
            self.scripts = [_script(96, (64, 65), (90, 96)) + _script(16, (0, 16)),
                            _script(96, (10, 64), (65, 70)) + _script(16),
                            _script(96, *many, (60, 70), (94, 96)) + _script(16, (0, 3))]
        else:
            raise ValueError(name)
        self.state0 = VadState(state.v)
        self.audio = script_audio(self.scripts, frame, 100 + frame + len(name))
        assert sum(self.cuts) == len(self.scripts[0])

    def chunks(self):
        """The scene's chunks, fp32 ``[B, cut * frame]`` each, contiguous."""
        out, at = [], 0
        for c in self.cuts:
            out.append(self.audio[:, at * self.frame:(at + c) * self.frame].contiguous())
            at += c
        return out


SCENES = [("bursts", f) for f in FRAMES] + [("sharp", SHARP_FRAME)]


@functools.lru_cache(maxsize=None)
def scene(name, frame):
    return Scene(name, frame)


@functools.lru_cache(maxsize=None)
def reference(name, frame):
    """``((mask, seg, count, speech, silent, level, zc, state_out), ...)`` of ``voice_activity_ref``,
    one per chunk; computed once, not to be modified."""
    from aiko_services_amd.ops.reference import voice_activity_ref
    s = scene(name, frame)
    state, steps = s.state0, []
    for chunk in s.chunks():
        out = voice_activity_ref(chunk, state, **s.kw)
        state = out[7]
        steps.append(out)
    return tuple(steps)


def whole_mask(name, frame):
    """The reference's mask over the whole scene, uint8 ``[B, F]``."""
    return torch.cat([step[0] for step in reference(name, frame)], dim=1)


def runs_of(mask_row):
    """[(first, one past last), ...] of a 0/1 sequence."""
    out, start = [], None
    m = [int(v) for v in mask_row]
    for f, v in enumerate(m + [0]):
        if v and start is None:
            start = f
        elif not v and start is not None:
            out.append((start, f))
            start = None
    return out


def assert_conditions():
    """What the scenes must exercise, asserted on the reference's own results, so that a scene cannot
    quietly stop exercising a rule."""
    from aiko_services_amd.ops.vad import FRAME_TILE
    for frame in FRAMES:
        s, ref = scene("bursts", frame), reference("bursts", frame)
        kw = s.kw
        assert max(s.cuts) <= 64 and any(c % FRAME_TILE for c in s.cuts)
        # the cut after chunk 0 is inside stream 0's attack run, the one after chunk 1 inside its hangover
        v0, v1 = ref[0][7].v[0], ref[1][7].v[0]
        assert 0 < int(v0[2]) < kw["attack"] and int(v0[4]) == 0
        assert int(v1[4]) == 1 and 0 < int(v1[3]) <= kw["hang"]
        whole = whole_mask("bursts", frame)
        # onset lags by attack - 1, the hangover is hang frames long; a burst shorter than attack is ignored
        a, h = kw["attack"], kw["hang"]
        assert runs_of(whole[0]) == [(8 + a - 1, 18 + h), (60 + a - 1, 75 + h), (110 + a - 1, 120)]
        # a hangover bridges the gap 8..12 once the first burst is on; the short one at 34 opens a run
        assert runs_of(whole[1]) == [(5 + a - 1, 14 + h), (34 + a - 1, 37 + h), (50 + a - 1, 100 + h)]
        # seen < 0 over garbage: the empty state
        assert int(s.state0.v[2, 1]) < 0 and int(ref[0][7].v[2, 1]) == s.cuts[0]
        assert runs_of(whole[2]) == [(20 + a - 1, 36 + h), (99 + a - 1, 104 + h)]
        assert [int(x) for x in ref[-1][7].v[:, 1]] == [120] * B
        # silent follows since >= window: stream 2 is silent from the start until its first burst
        assert [int(step[4][2]) for step in ref] == [1, 1, 0, 1, 0]
        # a run that continues from the chunk before starts at 0
        assert int(ref[2][1][0, 0, 0]) == 0 and int(ref[1][0][0, -1]) == 1
    s, ref = scene("sharp", SHARP_FRAME), reference("sharp", SHARP_FRAME)
    first, second = ref
    for b in range(B):                                      # attack 1, hang 0: the mask is the script
        assert [int(v) for v in whole_mask("sharp", SHARP_FRAME)[b]] == s.scripts[b], b
    assert first[0].shape[1] > 65
    assert first[0][0, 63:66].tolist() == [0, 1, 0] and first[0][1, 63:66].tolist() == [1, 0, 1]
    assert first[0][2, 60:70].all()                         # a run across the word boundary
    assert len(runs_of(first[0][2])) > s.kw["max_seg"] == int(first[2][2])      # more runs than rows
    assert first[1][2].tolist() == [[2, 3], [5, 6]]
    assert first[1][0].tolist() == [[64, 65], [90, 96]]     # ... a run that ends the chunk
    assert first[1][1].tolist() == [[10, 64], [65, 70]]
    assert second[0][0].all() and second[1][0].tolist() == [[0, 16], [0, 0]] and int(second[3][0]) == 16
    assert not second[0][1].any() and int(second[2][1]) == 0 and not second[1][1].any()
    assert second[1][2].tolist() == [[0, 3], [0, 0]] and int(second[2][2]) == 1
    assert second[4].tolist() == [0, 1, 1]                  # since: 0, 42 and 13 frames against a window of 8
