"""Coded frames for the JPEG decoder's tests, CPU and GPU: Pillow streams of the three samplings, the
project's own encoder's streams, hand-edited headers and corrupt streams, with their reference decodes
computed once and shared.  A plain module next to ``jpeg_scenes``: no fixtures, no device."""
from __future__ import annotations

import io
from functools import lru_cache

import numpy as np
import torch

import jpeg_scenes as S

FORMATS = ("i420", "yuyv", "i444")
SUBSAMPLING = {"i420": 2, "yuyv": 1, "i444": 0}            # Pillow's name for each
# the smallest shapes that can go wrong: one sample (two for yuyv); one MCU; partial MCUs on both edges
# with odd chroma planes; more than 8 intervals (the RST counter wraps); more blocks in an MCU row than
# lanes in a workgroup
SHAPES = ((1, 1), (8, 8), (16, 16), (17, 23), (152, 24), (16, 720))
KINDS = ("ours", "pillow", "pillow_rst1", "pillow_opt")
CORRUPT_SHAPE = ("i420", 48, 24)                          # 3 MCU rows of 2 MCUs: three intervals of ours


def width(fmt: str, W: int) -> int:
    """``W``, made even for yuyv (17 x 23 becomes 17 x 24, 1 x 1 becomes 1 x 2)."""
    return W + (W & 1) if fmt == "yuyv" else W


def pillow_stream(rgb: torch.Tensor, fmt: str, quality: int, **kw) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb.numpy(), "RGB").save(buf, format="JPEG", quality=quality, subsampling=SUBSAMPLING[fmt], **kw)
    return buf.getvalue()


def pillow_planes(data: bytes) -> np.ndarray:
    """Pillow's own decode of ``data`` without the colour conversion: ``[H, W, 3]`` Y, Cb, Cr (chroma
    upsampled by Pillow's rule)."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr", im.mode
    return np.asarray(im)


def rebuild(segments, rest: bytes) -> bytes:
    """A stream from ``(marker, body)`` segments (``jpeg_scenes.segments``) and what follows ``SOS``."""
    out = [b"\xff\xd8"]
    for marker, body in segments:
        out.append(bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body))
    return b"".join(out) + rest


def split(data: bytes):
    """``(segments, entropy-coded rest)`` of a stream."""
    segs = S.segments(data)
    head = 2 + sum(4 + len(body) for _, body in segs)
    return segs, data[head:]


def without_dht(data: bytes) -> bytes:
    segs, rest = split(data)
    return rebuild([s for s in segs if s[0] != 0xC4], rest)


def planes_of(raw: torch.Tensor, fmt: str, H: int, W: int):
    """``(y [H, W], u, v)`` numpy views of one raw frame."""
    a = raw.numpy()
    if fmt == "yuyv":
        p = a.reshape(H, W // 2, 4)
        return p[:, :, 0::2].reshape(H, W), p[:, :, 1], p[:, :, 3]
    ch, cw = ((H + 1) // 2, (W + 1) // 2) if fmt == "i420" else (H, W)
    return a[:H * W].reshape(H, W), a[H * W:H * W + ch * cw].reshape(ch, cw), a[H * W + ch * cw:].reshape(ch, cw)


@lru_cache(maxsize=None)
def streams(fmt: str, H: int, W: int, kind: str) -> tuple:
    """The coded frames (bytes) of one kind at one shape.  ``ours``: the three frames of
    ``jpeg_scenes.frames`` by ``jpeg_encode_ref`` at quality 90 (none for yuyv, which the encoder does not
    write); the Pillow kinds: a structured frame at quality 90 and a noise frame at quality 50."""
    if kind == "ours":
        if fmt == "yuyv":
            return ()
        stream, nbytes = S.reference(fmt, H, W, 90)
        return tuple(S.stream_bytes(stream, nbytes, b) for b in range(3))
    kw = {"pillow": {}, "pillow_rst1": {"restart_marker_blocks": 1}, "pillow_opt": {"optimize": True}}[kind]
    g = torch.Generator().manual_seed(H * 4099 + W)
    noise = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g)
    return (pillow_stream(S.structured_rgb(H, W), fmt, 90, **kw), pillow_stream(noise, fmt, 50, **kw))


@lru_cache(maxsize=None)
def packed(fmt: str, H: int, W: int, kind: str):
    """``(data, nbytes, desc, plan)`` of :func:`streams`."""
    from aiko_services_amd.ops import jpeg_decode as D
    return D.pack(list(streams(fmt, H, W, kind)))


@lru_cache(maxsize=None)
def reference(fmt: str, H: int, W: int, kind: str):
    """``(raw, status)`` of :func:`packed` by ``jpeg_decode_ref``."""
    from aiko_services_amd.ops.reference import jpeg_decode_ref
    data, nbytes, desc, _ = packed(fmt, H, W, kind)
    return jpeg_decode_ref(data, nbytes, desc, H, W, fmt)


# ---- corrupt streams --------------------------------------------------------------------------

def _status(frame: bytes, nbytes: int | None = None) -> int:
    from aiko_services_amd.ops import jpeg_decode as D
    from aiko_services_amd.ops.reference import jpeg_decode_ref
    fmt, H, W = CORRUPT_SHAPE
    plan = D.parse(frame)
    data = torch.frombuffer(bytearray(frame) + bytearray(8), dtype=torch.uint8)[None]
    n = torch.tensor([len(frame) if nbytes is None else nbytes], dtype=torch.int32)
    return int(jpeg_decode_ref(data, n, D.plan_bytes(plan)[None], H, W, fmt)[1][0])


def flip(frame: bytes, bit: int) -> bytes:
    out = bytearray(frame)
    out[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(out)


@lru_cache(maxsize=None)
def corrupt_handful() -> dict:
    """name -> ``(frame bytes, nbytes)``: a valid stream of :data:`CORRUPT_SHAPE` by the project's encoder
    (three intervals) and a fixed handful of corruptions of it.  ``nbytes`` may differ from the length."""
    from aiko_services_amd.ops import jpeg_decode as D
    fmt, H, W = CORRUPT_SHAPE
    stream, nbytes = S.reference(fmt, H, W, 90)
    good = S.stream_bytes(stream, nbytes, 2)               # the structured frame
    scan = D.parse(good).scan_offset
    marks = [i for i in range(scan, len(good) - 3) if good[i] == 0xFF and 0xD0 <= good[i + 1] <= 0xD7]
    assert len(marks) == 2
    out = {"valid": (good, len(good)), "truncated": (good[:len(good) - 9], len(good) - 9),
           "cut_short_with_eoi": (good[:marks[1] + 2 + 5] + b"\xff\xd9", marks[1] + 9),
           "removed_rst": (good[:marks[0]] + good[marks[0] + 2:], len(good) - 2),
           "swapped_rst": (good[:marks[0] + 1] + bytes([good[marks[1] + 1]]) + good[marks[0] + 2:marks[1] + 1] +
                           bytes([good[marks[0] + 1]]) + good[marks[1] + 2:], len(good)),
           "stray_marker": (good[:scan + 3] + b"\xff\xc4" + good[scan + 5:], len(good)),
           "zero_length": (good, 0), "overflowed_encode": (good, -1)}
    # the first single-bit flips of the entropy-coded bytes that end in each of these statuses
    wanted = {2: "invalid_code", 8: "run_leaves_block"}
    for bit in range(8 * scan, 8 * (len(good) - 2)):
        if not wanted:
            break
        bad = flip(good, bit)
        st = _status(bad)
        if st in wanted:
            out[wanted.pop(st)] = (bad, len(bad))
    return out


def pack_raw(frames, lengths, plan, cap=None):
    """``(data, nbytes, desc)`` of frames that ``pack`` would trim or refuse: the bytes as they are, the
    given ``nbytes``, one descriptor for all."""
    from aiko_services_amd.ops import jpeg_decode as D
    cap = cap or (max(len(f) for f in frames) + 63) // 64 * 64
    data = torch.zeros(len(frames), cap, dtype=torch.uint8)
    for k, f in enumerate(frames):
        if f:
            data[k, :len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8)
    desc = D.plan_bytes(plan)[None].repeat(len(frames), 1)
    return data, torch.tensor(list(lengths), dtype=torch.int32), desc
