"""Voice activity (``csrc/kernels/vad_ops.hip``): did anybody speak in this chunk, and when?  Batch
row ``b`` is one 16 kHz mono stream; its noise floor and counters are a :class:`VadState` in HBM, read
and rewritten once per chunk.  Out come a mask per frame of 10, 20 or 30 ms, its runs as segments and
one ``silent`` flag per stream, which ``WhisperDecoder.transcribe`` takes as the stream's ``done``.
Two launches, no host copy, no synchronisation, hipGraph-capturable like
:func:`~aiko_services_amd.ops.motion.motion_detect`.

The rule, per row.  After one exact fp32 scaling it is all integer, so
:func:`~aiko_services_amd.ops.reference.voice_activity_ref` (the same in plain loops) equals the
kernels bit for bit, and a signal cut into chunks gives what one call over all of it gives.

Parameters (defaults in brackets): ``frame`` 160, 320 or 480 samples [320: 20 ms]; ``threshold``
0..1023 level units [48: 3 octaves of power, 9 dB]; ``min_level`` 0..1023 [0]; ``up_shift`` [6],
``speech_shift`` [10] and ``down_shift`` [1], each 0..16; ``warmup`` >= 1 frames [10]; ``attack`` >= 1
[3]; ``hang`` >= 0 [15]; ``max_zc`` 0..479 [479: off]; ``window`` >= 1 frames [1500]; ``max_seg`` 1..64
[16].  ``audio`` is fp32 ``[B, n]``, contiguous, ``n % frame == 0``, ``F = n / frame``, ``1 <= F <=
4096``.

1. **Sample.**  ``v = x * 32768.0f`` (exact); ``q = 0`` if ``v`` is NaN, else ``(int) rintf(min(max(v,
   -32768), 32767))``, round half to even; +-inf clamp.
2. **Frame.**  Frames do not overlap and are ``frame`` samples long.  ``E = sum of q*q`` in 64 bits
   (480 samples at -1.0 give 480 * 2^30).  ``z`` is the number of ``i`` in ``1..frame-1`` with ``(q[i]
   < 0) != (q[i-1] < 0)``: the sign of ``q``, not of ``x`` (-1e-6 quantises to 0, which is not
   negative), and within the frame, so frames are independent.
3. **Level.**  ``level = 0`` if ``E == 0``.  Else ``p = floor(log2 E)``, ``mant = (E >> (p-4)) & 15`` if
   ``p >= 4`` else ``(E << (4-p)) & 15``, ``level = 16*(p+1) + mant``: a piecewise-linear log2 in
   sixteenths of an octave of power, 0..639.  A full-scale 440 Hz sine at frame 320 is 612.
4. **State.**  :class:`VadState` ``v`` int32 ``[B, 8]``, columns ``floor, seen, run, quiet, on, since,
   0, 0``; the empty state is zeros.  ``floor`` is in 256ths of a level unit.  ``s = max(seen, 0)``.
   If ``s == 0`` at the start of a call the row is the empty state whatever its columns hold: ``run =
   quiet = on = 0`` and ``since = 2^30`` (``floor`` is set by the first frame).  Otherwise ``on`` is
   read as ``on != 0``, ``run`` and ``since`` clamped to ``0..2^30``, ``quiet`` to ``>= 0`` and ``floor``
   to ``0..1023 << 8``, which changes nothing in a state the rule wrote (the floor moves towards
   ``cur`` and never past it) and keeps every difference within 32 bits.
5. **Per frame, in order.**  ``cur = level << 8``.

   * If ``s == 0``: ``floor = cur``.
   * ``raw = s >= warmup and level >= min_level and cur - floor > (threshold << 8) and z <= max_zc``,
     against the floor before its update.
   * If ``s > 0``: ``k = down_shift`` if ``cur < floor``, else ``speech_shift`` if ``raw``, else
     ``up_shift``; ``floor += (cur - floor + half(k)) >> k``, the shift arithmetic (floor), ``half(k) =
     1 << (k-1)``, ``half(0) = 0``.
   * ``run = min(run+1, 2^30)`` if ``raw`` else 0.
   * If ``on == 0``: ``run >= attack`` sets ``on = 1, quiet = 0``.  Else ``quiet = 0`` if ``raw`` else
     ``quiet + 1``, and ``quiet > hang`` sets ``on = 0, quiet = 0``.
   * ``mask[f] = on``; ``since = 0`` if ``on`` else ``min(since+1, 2^30)``; ``s = min(s+1, 2^31-1)``.

   The onset lags by ``attack - 1`` frames and the hangover is part of the speech: that is the rule.
6. **Outputs.**  ``level``, ``zc`` int32 ``[B, F]``; ``mask`` uint8 ``[B, F]``; ``seg`` int32 ``[B,
   max_seg, 2]``, the maximal runs of ``mask == 1`` in the chunk, in order, as ``(first frame, one past
   the last)``: only the first ``max_seg`` are kept, rows at or past ``count`` are zeros, a run that
   continues from the chunk before starts at 0; ``count`` int32 ``[B]``, the rows written; ``speech``
   int32 ``[B]``, the sum of ``mask``; ``silent`` int32 ``[B]``, 1 iff ``since >= window`` after the
   last frame; ``state_out``.  Every element of every output is written.

What the defaults do, on 12 s of noise at 0.02 with a 0.3 tone at 2..3.5 s, a 40 ms blip, a 0.05 tone
and a 12 dB step of the noise: the tone is one segment at every ``frame``; the 0.05 tone is ignored;
the blip is ignored at frames 320 and 480 and is one short segment at frame 160, where its four
frames meet ``attack`` = 3.  The noise step reads as speech, and the floor absorbs it only slowly,
over seconds: while ``raw`` holds the floor follows at ``speech_shift``, 1/1024 of the distance per
frame.  That is the price of a floor that speech does not drag up; a shorter ``speech_shift`` trades
one for the other.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

__all__ = ["DEFAULTS", "FRAMES", "FRAME_TILE", "MAX_FRAMES", "VadState", "check_parameters", "frame_grid",
           "new_state", "vad_uses_vector", "voice_activity"]

FRAMES = (160, 320, 480)
MAX_FRAMES = 4096              # frames per call and stream (VA_MAX_F)
FRAME_TILE = 4                 # frames per workgroup of the frame pass (VA_WAVES)
DEFAULTS = dict(frame=320, threshold=48, min_level=0, up_shift=6, speech_shift=10, down_shift=1, warmup=10,
                attack=3, hang=15, max_zc=479, window=1500, max_seg=16)


class VadState(NamedTuple):
    """``v`` int32 ``[B, 8]``: ``floor`` (256ths of a level unit), ``seen``, ``run``, ``quiet``, ``on``,
    ``since``, 0, 0 per stream."""
    v: torch.Tensor


def new_state(B: int, device="cuda") -> VadState:
    """The empty state of ``B`` streams: zeros."""
    return VadState(torch.zeros(int(B), 8, dtype=torch.int32, device=device))


def check_parameters(frame=320, threshold=48, min_level=0, up_shift=6, speech_shift=10, down_shift=1, warmup=10,
                     attack=3, hang=15, max_zc=479, window=1500, max_seg=16) -> None:
    """The value ranges of the rule's parameters, as ``ValueError``."""
    if isinstance(frame, bool) or frame not in FRAMES:
        raise ValueError(f"voice_activity: frame one of {FRAMES} required, got {frame!r}")
    top = 2 ** 31 - 1
    for name, v, lo, hi in (("threshold", threshold, 0, 1023), ("min_level", min_level, 0, 1023),
                            ("up_shift", up_shift, 0, 16), ("speech_shift", speech_shift, 0, 16),
                            ("down_shift", down_shift, 0, 16), ("warmup", warmup, 1, top), ("attack", attack, 1, top),
                            ("hang", hang, 0, top), ("max_zc", max_zc, 0, 479), ("window", window, 1, top),
                            ("max_seg", max_seg, 1, 64)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"voice_activity: {name} an integer in {lo}..{hi} required, got {v!r}")


def vad_uses_vector(audio: torch.Tensor) -> bool:
    """Whether the ``float4`` frame pass serves this ``audio``: 16-byte aligned (a row is whole frames
    of 160, 320 or 480 floats, so every frame then is); every other call runs the scalar kernel."""
    return audio.data_ptr() % 16 == 0


def frame_grid(F: int, batch: int) -> tuple[int, int]:
    """The frame pass's grid: ``ceil(F / FRAME_TILE)`` tiles of frames times ``batch`` streams."""
    return (int(F) + FRAME_TILE - 1) // FRAME_TILE, int(batch)


def voice_activity(audio: torch.Tensor, state: VadState, *, frame: int = 320, threshold: int = 48, min_level: int = 0,
                   up_shift: int = 6, speech_shift: int = 10, down_shift: int = 1, warmup: int = 10, attack: int = 3,
                   hang: int = 15, max_zc: int = 479, window: int = 1500, max_seg: int = 16,
                   state_out: VadState | None = None, level: torch.Tensor | None = None,
                   zc: torch.Tensor | None = None, mask: torch.Tensor | None = None, seg: torch.Tensor | None = None,
                   count: torch.Tensor | None = None, speech: torch.Tensor | None = None,
                   silent: torch.Tensor | None = None):
    """One chunk: fp32 ``[B, n]`` ``audio`` and ``state`` -> ``(mask, seg, count, speech, silent, level,
    zc, state_out)`` (the rule: this module's docstring).  ``state`` is only read; ``state_out`` (new by
    default) must be another allocation.  Parameters out of range are a ``ValueError``; shapes, dtypes,
    devices, overlap, ``n % frame`` and ``F > 4096`` are refused by the operator."""
    check_parameters(frame, threshold, min_level, up_shift, speech_shift, down_shift, warmup, attack, hang, max_zc,
                     window, max_seg)
    if audio.dim() != 2:
        raise ValueError(f"voice_activity: audio [B, n] required, got {tuple(audio.shape)}")
    B, n = audio.shape
    F = n // int(frame)
    dev = audio.device
    if state_out is None:
        state_out = VadState(torch.empty(B, 8, dtype=torch.int32, device=dev))
    level, zc = (torch.empty(B, F, dtype=torch.int32, device=dev) if t is None else t for t in (level, zc))
    if mask is None:
        mask = torch.empty(B, F, dtype=torch.uint8, device=dev)
    if seg is None:
        seg = torch.empty(B, int(max_seg), 2, dtype=torch.int32, device=dev)
    elif seg.dim() != 3 or seg.shape[1] != int(max_seg):
        raise ValueError(f"voice_activity: seg [B, max_seg = {max_seg}, 2] required, got {tuple(seg.shape)}")
    count, speech, silent = (torch.empty(B, dtype=torch.int32, device=dev) if t is None else t
                             for t in (count, speech, silent))
    torch.ops.aiko.voice_activity_out(audio, state.v, int(frame), int(threshold), int(min_level), int(up_shift),
                                      int(speech_shift), int(down_shift), int(warmup), int(attack), int(hang),
                                      int(max_zc), int(window), state_out.v, level, zc, mask, seg, count, speech,
                                      silent)
    return mask, seg, count, speech, silent, level, zc, state_out
