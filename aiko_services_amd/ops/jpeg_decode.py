"""Baseline JPEG decoding on the device (``csrc/kernels/jpeg_decode_ops.hip``), the inverse of
:mod:`~aiko_services_amd.ops.jpeg`: complete JPEG streams in HBM, one per batch row -> tightly packed
raw frames in HBM, which ``yuv_to_rgb(..., standard="jpeg")`` turns into RGB.  Three launches, no host
copy, no synchronisation, no allocation when the outputs and the workspace are given:
hipGraph-capturable.  The rule is all integer, so
:func:`~aiko_services_amd.ops.reference.jpeg_decode_ref` (the same in plain loops) equals the kernels
bit for bit.  The host's share is the header: :func:`parse` reads it, :func:`plan_bytes` lays it out
for the device, :func:`pack` does both for a batch of coded frames.

**Streams taken.**  Baseline sequential DCT (``SOF0``), 8-bit samples, one interleaved scan of exactly
three components with ``Ss = 0, Se = 63, Ah = Al = 0``.  Sampling factors ``2x2, 1x1, 1x1`` decode to
the raw format ``i420``, ``2x1, 1x1, 1x1`` to ``yuyv`` (the width must be even, as
:func:`~aiko_services_amd.ops.yuv.frame_bytes` demands), ``1x1, 1x1, 1x1`` to ``i444``.  Any 8-bit
``DQT``, any ``DHT`` with ids 0 and 1, any ``DRI`` including none; ``APPn`` and ``COM`` segments are
skipped.  A stream with no ``DHT`` at all gets the Annex K tables :data:`~aiko_services_amd.ops.jpeg.HUFFMAN`
(the MJPG-in-AVI convention).  ``1 <= H <= 65535``, ``1 <= W <= 4096``.  Everything else raises
:class:`JpegUnsupported` (a ``ValueError``) with the reason in words, so that a caller can fall back to
another decoder: progressive streams, ``SOF1``, ``SOF9`` and the other frame types, 12-bit samples,
grayscale and 4 components, other sampling factors, several scans, 16-bit ``DQT``, a table referenced
but never defined, ``yuyv`` with an odd width.

An MCU is 16 x 16 luma for ``i420`` (blocks Y00 Y01 Y10 Y11 Cb Cr), 16 x 8 for ``yuyv`` (Y0 Y1 Cb Cr)
and 8 x 8 for ``i444`` (Y Cb Cr); ``mx = ceil(W / mcu_w)``, ``my = ceil(H / mcu_h)``, ``mcus = mx * my``.

**Restart intervals.**  ``intervals = ceil(mcus / DRI)``, or 1 without ``DRI``.  Interval ``i`` is the
bytes between ``RST(i-1)`` and ``RST(i)``; the first starts at the end of ``SOS``, the last ends at
``EOI``, which must sit at ``nbytes - 2``.  A restart marker is a byte pair ``FF Dm``, ``0 <= m <= 7``,
that lies wholly inside ``[scan offset, nbytes - 2)``.  They must number exactly ``intervals - 1`` and
carry ``m = i mod 8`` in order.  Interval ``i`` holds the MCUs ``[i * DRI, min((i + 1) * DRI, mcus))`` in
raster order.

**Entropy decoding.**  Standard baseline decoding: the canonical codes of Annex C (``DECODE`` of
Annex F: the first length ``l`` at which the ``l`` bits read so far are at most ``maxcode[l]``), the DC
difference per component, the predictors 0 at the start of every restart interval, after each
addition clamped to int16 range (a valid stream never reaches the clamp).  The size of a DC
difference is the low four bits of its symbol.  For an AC symbol ``r << 4 | s``: ``s > 0`` skips ``r``
zeros and reads ``s`` value bits; ``ZRL`` (0xF0) skips 16; every other symbol with ``s = 0`` ends the
block, as ``EOB`` (0x00) does.  ``EXTEND`` follows the standard.  Bits are taken MSB first; inside an
interval ``FF 00`` is the byte ``FF``.

**Errors are data, never a fault.**  Each frame has a status, 0 for success, otherwise the OR of

    1   marker count or order wrong, no ``EOI`` at ``nbytes - 2``, ``nbytes <= 0`` or beyond the row,
        the scan offset outside the stream, or more intervals than the call allows
    2   sixteen bits that are no code in the table
    4   a bit needed past the interval's end
    8   a run that leaves the block (a coefficient index above 63, or a ``ZRL`` with fewer than 16
        coefficients left)
    16  a bit needed from an ``FF`` that is followed by anything but ``00`` inside the interval

over the frame's intervals and its marker scan.  An interval stops at its first error; a frame whose
marker scan fails (bit 1) is not decoded at all.  Bytes of an interval that the decoder never needs
are not looked at: a valid stream leaves bits unread only in the final byte of an interval.  A frame
with a non-zero status has unspecified bytes within its own output row; every other frame is
unaffected.

**Dequantisation and inverse DCT, integers only**, the mirror of the encoder's forward rule:
``c = clamp(v * q, -2048, 2047)``; with ``M`` = :data:`~aiko_services_amd.ops.jpeg.DCT_MATRIX`, columns
first, ``t = (M^T @ c + 1024) >> 11``, then rows, ``x = (t @ M + 16384) >> 15``; the sample is
``clamp(x + 128, 0, 255)``.  The shifts are arithmetic and any summation order gives the same bits.
int32 suffices: the largest absolute row or column sum of ``M`` is 23168, ``2048 * 23168 < 2^26`` for
the first pass and ``23169 * 23168 < 2^30`` for the second.  Samples outside a component's plane (the
partial MCUs at the right and bottom edges) are dropped.

**Output.**  The tightly packed raw frame of ``frame_bytes(fmt, H, W)``, full range, chroma
centre-sited: what ``yuv_to_rgb(..., standard="jpeg")`` reads and ``rgb_to_yuv(..., standard="jpeg")``
writes.  RGB is ``yuv_to_rgb`` behind the decode, chroma replicated as that operator defines.

**The device descriptor** of one header, :data:`PLAN_BYTES` = 1744 bytes, little endian::

    0     int32     scan offset: the first byte behind SOS
    4     int32     DRI, 0 for none
    8     uint8[3]  slot (0 | 1) of each component's DC table;  11  uint8[3]  ... of its AC table
    16    uint8[3][64]   the components' quantisers, natural (row-major) order
    208   four Huffman tables of 384 bytes: DC slot 0, DC slot 1, AC slot 0, AC slot 1, each
          int32[16]  maxcode of the lengths 1..16, -1 for a length without codes
          int32[16]  valoff: symbols[code + valoff[l]] is the symbol of a code of length l
          uint8[256] the symbols in code order

A slot no component uses holds ``maxcode`` -1 throughout.

**The workspace** (:func:`workspace_bytes`), 16-byte aligned: int32 ``[B]`` marker-scan status, int32
``[B, max_intervals]`` interval starts, int32 ``[B, max_intervals]`` interval statuses, padding to 16
bytes, then int16 ``[B, blocks, 64]`` coefficients in zigzag order.  ``max_intervals`` follows from the
``restart_interval`` a call names (``None``: the worst case, one MCU per interval); a frame whose own
``DRI`` gives more intervals than that has status bit 1.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from . import jpeg as _J
from .yuv import FORMATS, frame_bytes

__all__ = ["DECODE_FORMATS", "JpegPlan", "JpegUnsupported", "PLAN_BYTES", "blocks", "intervals", "jpeg_decode", "pack",
           "parse", "plan_bytes", "workspace_bytes"]

#: raw format -> (MCU height, MCU width, blocks per MCU)
DECODE_FORMATS = {"i420": (16, 16, 6), "yuyv": (8, 16, 4), "i444": (8, 8, 3)}
#: the luminance component's (H, V) sampling factors -> raw format (chroma is 1x1 throughout)
_SAMPLING = {(2, 2): "i420", (2, 1): "yuyv", (1, 1): "i444"}
PLAN_BYTES = 1744
_P_SEL, _P_Q, _P_HUFF, _P_HUFF_BYTES = 8, 16, 208, 384
MAX_WIDTH, MAX_HEIGHT = _J.MAX_WIDTH, _J.MAX_HEIGHT

_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)",
              0xC5: "differential sequential (SOF5)", 0xC6: "differential progressive (SOF6)",
              0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic-coded sequential (SOF9)",
              0xCA: "arithmetic-coded progressive (SOF10)", 0xCB: "arithmetic-coded lossless (SOF11)",
              0xCD: "arithmetic-coded differential sequential (SOF13)",
              0xCE: "arithmetic-coded differential progressive (SOF14)",
              0xCF: "arithmetic-coded differential lossless (SOF15)"}


class JpegUnsupported(ValueError):
    """A stream the device decoder does not take; the message says why."""


@dataclass(frozen=True)
class JpegPlan:
    """What a header says: the raw format and size the stream decodes to, ``restart_interval`` (0: none),
    ``scan_offset`` (the first byte behind ``SOS``), per component the quantiser (64 ints, natural
    order) and the DC and AC Huffman table as ``(codes per length 1..16, symbols in code order)``, and
    the table ids (0 | 1) the scan header gives each component."""
    fmt: str
    height: int
    width: int
    restart_interval: int
    scan_offset: int
    quant: tuple
    dc: tuple
    ac: tuple
    dc_ids: tuple
    ac_ids: tuple


def geometry(fmt: str, height: int, width: int) -> tuple:
    """``(mcu_h, mcu_w, blocks per MCU, my, mx)``; ``ValueError`` for anything the decoder does not write."""
    if fmt not in DECODE_FORMATS:
        raise ValueError(f"jpeg_decode: format {fmt!r} cannot be decoded to (one of {sorted(DECODE_FORMATS)})")
    for v in (height, width):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"jpeg_decode: height and width integers required, got {height!r} x {width!r}")
    h, w = int(height), int(width)
    if not (1 <= h <= MAX_HEIGHT and 1 <= w <= MAX_WIDTH):
        raise ValueError(f"jpeg_decode: 1 <= height <= {MAX_HEIGHT} and 1 <= width <= {MAX_WIDTH} required, "
                         f"got {h} x {w}")
    if fmt == "yuyv" and w % 2:
        raise ValueError(f"jpeg_decode: yuyv needs an even width, got {w}")
    mh, mw, nb = DECODE_FORMATS[fmt]
    return mh, mw, nb, -(-h // mh), -(-w // mw)


def blocks(fmt: str, height: int, width: int) -> int:
    """8 x 8 blocks a frame codes."""
    _, _, nb, my, mx = geometry(fmt, height, width)
    return nb * my * mx


def intervals(fmt: str, height: int, width: int, restart_interval: int | None) -> int:
    """Restart intervals of a frame: ``ceil(mcus / restart_interval)``, 1 for 0 (no ``DRI``), ``mcus`` for
    ``None`` (the most a frame can have)."""
    _, _, _, my, mx = geometry(fmt, height, width)
    if restart_interval is None:
        return my * mx
    if isinstance(restart_interval, bool) or int(restart_interval) != restart_interval or \
            not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"jpeg_decode: restart_interval an integer in 0..65535 or None required, got "
                         f"{restart_interval!r}")
    ri = int(restart_interval)
    return -(-(my * mx) // ri) if ri else 1


def workspace_bytes(fmt: str, height: int, width: int, batch: int, restart_interval: int | None = None) -> int:
    """Bytes of the workspace of a call (its layout: the module docstring)."""
    n = intervals(fmt, height, width, restart_interval)
    ints = int(batch) * (1 + 2 * n)
    return (4 * ints + 15) // 16 * 16 + int(batch) * blocks(fmt, height, width) * 128


# ---- the header ---------------------------------------------------------------------------------

def _header_end(data) -> int:
    """Offset of the first byte behind ``SOS``; :class:`JpegUnsupported` if the segments do not lead there."""
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise JpegUnsupported("jpeg: no SOI marker at the start: not a JPEG stream")
    i = 2
    while True:
        if i + 4 > n:
            raise JpegUnsupported("jpeg: the header ends before a scan header (SOS)")
        if data[i] != 0xFF:
            raise JpegUnsupported(f"jpeg: byte {i} of the header is not a marker")
        if data[i + 1] == 0xFF:                             # fill byte in front of a marker
            i += 1
            continue
        marker, length = data[i + 1], data[i + 2] << 8 | data[i + 3]
        if marker == 0xD9 or 0xD0 <= marker <= 0xD7 or marker == 0x01 or length < 2:
            raise JpegUnsupported(f"jpeg: marker FF {marker:02X} in the header, before any scan")
        i += 2 + length
        if i > n:
            raise JpegUnsupported("jpeg: the header ends inside a segment")
        if marker == 0xDA:
            return i


def _check_huffman(counts, symbols, what: str) -> None:
    code = 0
    for length in range(1, 17):
        code += counts[length - 1]
        if code > 1 << length:
            raise JpegUnsupported(f"jpeg: {what} assigns more codes of length {length} than there are")
        code <<= 1
    if len(symbols) != sum(counts) or len(symbols) > 256:
        raise JpegUnsupported(f"jpeg: {what} is cut short")


@lru_cache(maxsize=256)
def _parse_header(head: bytes) -> JpegPlan:
    quant, huff, frame, dri, scan, i = {}, {}, None, 0, None, 2
    while i < len(head):
        if head[i + 1] == 0xFF:
            i += 1
            continue
        marker, length = head[i + 1], head[i + 2] << 8 | head[i + 3]
        body = head[i + 4:i + 2 + length]
        i += 2 + length
        if marker == 0xDB:
            while body:
                pq, tq = body[0] >> 4, body[0] & 15
                if pq:
                    raise JpegUnsupported("jpeg: 16-bit quantisation table (DQT)")
                if tq > 3 or len(body) < 65:
                    raise JpegUnsupported("jpeg: malformed DQT segment")
                table = [0] * 64
                for z, n in enumerate(_J.ZIGZAG):
                    table[n] = body[1 + z]
                if min(table) < 1:
                    raise JpegUnsupported("jpeg: a quantiser of 0 in DQT")
                quant[tq] = tuple(table)
                body = body[65:]
        elif marker == 0xC4:
            while body:
                tc, th = body[0] >> 4, body[0] & 15
                if tc > 1 or th > 1 or len(body) < 17:
                    raise JpegUnsupported(f"jpeg: Huffman table class {tc} id {th}: ids 0 and 1 are taken")
                counts = tuple(body[1:17])
                symbols = tuple(body[17:17 + sum(counts)])
                _check_huffman(counts, symbols, f"Huffman table {body[0]:#04x}")
                huff[tc << 4 | th] = (counts, symbols)
                body = body[17 + sum(counts):]
        elif marker == 0xC0:
            if frame is not None:
                raise JpegUnsupported("jpeg: two frame headers")
            if len(body) < 6:
                raise JpegUnsupported("jpeg: malformed frame header")
            precision, height, width, nf = body[0], body[1] << 8 | body[2], body[3] << 8 | body[4], body[5]
            if precision != 8:
                raise JpegUnsupported(f"jpeg: {precision}-bit samples (8-bit only)")
            if nf == 1:
                raise JpegUnsupported("jpeg: grayscale stream (three components only)")
            if nf != 3 or len(body) < 6 + 3 * nf:
                raise JpegUnsupported(f"jpeg: {nf} components (three only)")
            comps = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(3)]
            frame = (height, width, comps)
        elif marker in _SOF_NAMES:
            bits = f", {body[0]}-bit samples" if body and body[0] != 8 else ""
            raise JpegUnsupported(f"jpeg: {_SOF_NAMES[marker]} stream{bits} (baseline SOF0 only)")
        elif marker == 0xDD:
            if len(body) < 2:
                raise JpegUnsupported("jpeg: malformed DRI segment")
            dri = body[0] << 8 | body[1]
        elif marker == 0xDA:
            scan = body
        elif marker == 0xDC:
            raise JpegUnsupported("jpeg: DNL segment (the height must stand in the frame header)")
        # APPn, COM and everything else: skipped
    if frame is None:
        raise JpegUnsupported("jpeg: no frame header (SOF0) in front of the scan")
    height, width, comps = frame
    sampling = tuple((h, v) for _, h, v, _ in comps)
    if sampling[1:] != ((1, 1), (1, 1)) or sampling[0] not in _SAMPLING:
        raise JpegUnsupported("jpeg: sampling factors " + ", ".join(f"{h}x{v}" for h, v in sampling) +
                              " (2x2, 2x1 or 1x1 luminance over 1x1 chrominance only)")
    fmt = _SAMPLING[sampling[0]]
    if not (1 <= height <= MAX_HEIGHT and 1 <= width <= MAX_WIDTH):
        raise JpegUnsupported(f"jpeg: size {height} x {width} (1..{MAX_HEIGHT} x 1..{MAX_WIDTH} only)")
    if fmt == "yuyv" and width % 2:
        raise JpegUnsupported(f"jpeg: 4:2:2 stream of odd width {width} (yuyv needs an even width)")
    if len(scan) < 1 or scan[0] != 3 or len(scan) < 10:
        ns = scan[0] if scan else 0
        raise JpegUnsupported(f"jpeg: a scan of {ns} of the 3 components: several scans (one interleaved scan only)")
    if (scan[7], scan[8], scan[9]) != (0, 63, 0):
        raise JpegUnsupported(f"jpeg: scan with Ss = {scan[7]}, Se = {scan[8]}, Ah/Al = {scan[9]:#04x} "
                              "(0, 63, 0 only)")
    dc_ids, ac_ids = [], []
    for c in range(3):
        if scan[1 + 2 * c] != comps[c][0]:
            raise JpegUnsupported("jpeg: the scan lists the components in another order than the frame header")
        td, ta = scan[2 + 2 * c] >> 4, scan[2 + 2 * c] & 15
        if td > 1 or ta > 1:
            raise JpegUnsupported(f"jpeg: the scan names Huffman table {max(td, ta)}: ids 0 and 1 are taken")
        dc_ids.append(td)
        ac_ids.append(ta)
    if not huff:
        huff = dict(_J.HUFFMAN)                            # no DHT at all: the MJPG-in-AVI convention
    for c in range(3):
        if comps[c][3] not in quant:
            raise JpegUnsupported(f"jpeg: quantisation table {comps[c][3]} referenced but never defined")
        for tc, ids in ((0, dc_ids), (1, ac_ids)):
            if tc << 4 | ids[c] not in huff:
                raise JpegUnsupported(f"jpeg: Huffman table {tc << 4 | ids[c]:#04x} referenced but never defined")
    return JpegPlan(fmt, height, width, dri, len(head), tuple(quant[comps[c][3]] for c in range(3)),
                    tuple(huff[dc_ids[c]] for c in range(3)), tuple(huff[0x10 | ac_ids[c]] for c in range(3)),
                    tuple(dc_ids), tuple(ac_ids))


def _as_bytes(data) -> bytes:
    if isinstance(data, torch.Tensor):
        data = data.cpu().numpy()
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise ValueError(f"jpeg: a coded frame is bytes or a 1-D uint8 array, got {data.dtype} {data.shape}")
        return data.tobytes()
    return bytes(data)


def parse(data) -> JpegPlan:
    """The :class:`JpegPlan` of a stream (bytes-like or a 1-D uint8 array; only the header, ``SOI`` up
    to the end of ``SOS``, is read).  Cached on the header's bytes: an MJPG stream repeats them frame
    after frame, so the cost per frame is a walk over the segment lengths and a dictionary lookup.
    :class:`JpegUnsupported` for a stream outside the rule of the module docstring."""
    if not isinstance(data, (bytes, bytearray)):
        data = _as_bytes(data)
    end = _header_end(data)
    return _parse_header(bytes(data[:end]))


def _huffman_words(counts, symbols) -> bytes:
    maxcode, valoff, code, k = [], [], 0, 0
    for length in range(1, 17):
        n = counts[length - 1]
        valoff.append(k - code)
        maxcode.append(code + n - 1 if n else -1)
        code, k = (code + n) << 1, k + n
    return struct.pack("<16i16i", *maxcode, *valoff) + bytes(symbols) + bytes(256 - len(symbols))


@lru_cache(maxsize=256)
def _plan_bytes(plan: JpegPlan) -> bytes:
    empty = struct.pack("<16i16i", *([-1] * 16), *([0] * 16)) + bytes(256)
    slots = [empty] * 4
    for c in range(3):
        slots[plan.dc_ids[c]] = _huffman_words(*plan.dc[c])
        slots[2 + plan.ac_ids[c]] = _huffman_words(*plan.ac[c])
    out = struct.pack("<ii", plan.scan_offset, plan.restart_interval) + bytes(plan.dc_ids) + bytes(plan.ac_ids) + \
        bytes(2) + b"".join(bytes(q) for q in plan.quant) + b"".join(slots)
    assert len(out) == PLAN_BYTES
    return out


def plan_bytes(plan: JpegPlan) -> torch.Tensor:
    """uint8 ``[PLAN_BYTES]``: the device descriptor of one header (the layout: the module docstring)."""
    return torch.frombuffer(bytearray(_plan_bytes(plan)), dtype=torch.uint8)


def pack(frames, out=None):
    """A batch of coded frames (a list of B bytes-like objects or 1-D uint8 arrays) -> ``(data uint8
    [B, cap], nbytes int32 [B], desc uint8 [B, PLAN_BYTES], plan)``, host tensors; ``plan`` is the first
    frame's.  ``out``: ``(data, nbytes, desc)`` to write into (pinned memory, say), ``data`` of any ``cap``
    that holds the longest frame; by default new tensors with ``cap`` the longest frame's length
    rounded up to 64.  Bytes behind the last ``FF D9`` are trimmed (AVI chunks are padded).  All frames
    must agree on ``(fmt, H, W)``, else ``ValueError``; their tables may differ.  An unsupported frame
    raises :class:`JpegUnsupported`."""
    if not isinstance(frames, (list, tuple)) or not frames:
        raise ValueError("jpeg pack: a non-empty list of coded frames required")
    raws, plans = [], []
    for k, f in enumerate(frames):
        b = _as_bytes(f)
        end = b.rfind(b"\xff\xd9")
        if end >= 0:
            b = b[:end + 2]
        plan = parse(b)
        if plans and (plan.fmt, plan.height, plan.width) != (plans[0].fmt, plans[0].height, plans[0].width):
            raise ValueError(f"jpeg pack: frame {k} is {plan.fmt} {plan.height} x {plan.width}, frame 0 "
                             f"{plans[0].fmt} {plans[0].height} x {plans[0].width}: one format and size per batch")
        raws.append(b)
        plans.append(plan)
    B, longest = len(raws), max(len(b) for b in raws)
    if out is None:
        cap = (longest + 63) // 64 * 64
        data = torch.zeros(B, cap, dtype=torch.uint8)
        nbytes = torch.empty(B, dtype=torch.int32)
        desc = torch.empty(B, PLAN_BYTES, dtype=torch.uint8)
    else:
        data, nbytes, desc = out
        ok = all(isinstance(t, torch.Tensor) and t.device.type == "cpu" and t.is_contiguous() for t in out)
        if not ok or data.dtype != torch.uint8 or data.dim() != 2 or data.shape[0] != B or \
                nbytes.dtype != torch.int32 or tuple(nbytes.shape) != (B,) or \
                desc.dtype != torch.uint8 or tuple(desc.shape) != (B, PLAN_BYTES):
            raise ValueError(f"jpeg pack: out = (data uint8 [{B}, cap], nbytes int32 [{B}], desc uint8 "
                             f"[{B}, {PLAN_BYTES}]) contiguous host tensors required")
        if data.shape[1] < longest:
            raise ValueError(f"jpeg pack: a frame of {longest} bytes does not fit data's cap = {data.shape[1]}")
    rows, lengths, drows = data.numpy(), nbytes.numpy(), desc.numpy()
    for k, (b, plan) in enumerate(zip(raws, plans)):
        rows[k, :len(b)] = np.frombuffer(b, np.uint8)
        lengths[k] = len(b)
        drows[k] = np.frombuffer(_plan_bytes(plan), np.uint8)
    return data, nbytes, desc, plans[0]


def jpeg_decode(data: torch.Tensor, nbytes: torch.Tensor, desc: torch.Tensor, height: int, width: int,
                fmt: str = "i420", *, restart_interval: int | None = None, raw: torch.Tensor | None = None,
                status: torch.Tensor | None = None, workspace: torch.Tensor | None = None):
    """Device ``data`` uint8 ``[B, cap]``, ``nbytes`` int32 ``[B]``, ``desc`` uint8 ``[B, PLAN_BYTES]`` or
    ``[1, PLAN_BYTES]`` (one header serving every frame: a shared header, or ``plan_bytes(parse(
    ops.jpeg.header(fmt, H, W, quality)))`` behind ``jpeg_encode`` on the device) -> ``(raw uint8 [B,
    frame_bytes(fmt, height, width)], status int32 [B])`` by the rule of the module docstring.  A frame
    with ``nbytes[b] <= 0`` (an overflowed encode) has status bit 1.  ``restart_interval`` bounds the
    intervals per frame the launches provide for (``None``: any stream; a plan's ``restart_interval``
    launches no idle lanes); ``workspace`` is uint8, 16-byte aligned, of at least
    :func:`workspace_bytes` bytes for the same ``restart_interval``.  Formats and sizes out of range are
    a ``ValueError``; dtypes, devices, contiguity, alignment and overlap are refused by the operator."""
    geometry(fmt, height, width)
    H, W = int(height), int(width)
    if data.dim() != 2 or nbytes.dim() != 1 or nbytes.shape[0] != data.shape[0]:
        raise ValueError(f"jpeg_decode: data [B, cap] and nbytes [B] required, got {tuple(data.shape)} and "
                         f"{tuple(nbytes.shape)}")
    B = data.shape[0]
    if desc.dim() != 2 or desc.shape[0] not in (1, B) or desc.shape[1] != PLAN_BYTES:
        raise ValueError(f"jpeg_decode: desc [{B}, {PLAN_BYTES}] or [1, {PLAN_BYTES}] required, got {tuple(desc.shape)}")
    max_intervals = intervals(fmt, H, W, restart_interval)
    need = frame_bytes(fmt, H, W)
    if raw is None:
        raw = torch.empty(B, need, dtype=torch.uint8, device=data.device)
    elif raw.dim() != 2 or tuple(raw.shape) != (B, need):
        raise ValueError(f"jpeg_decode: raw [{B}, {need}] required for {fmt} {H} x {W}, got {tuple(raw.shape)}")
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=data.device)
    if workspace is None:
        workspace = torch.empty(workspace_bytes(fmt, H, W, B, restart_interval), dtype=torch.uint8, device=data.device)
    torch.ops.aiko.jpeg_decode_out(data, nbytes, desc, H, W, FORMATS[fmt], max_intervals, raw, status, workspace)
    return raw, status
