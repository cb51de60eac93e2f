"""Baseline JPEG on the device (``csrc/kernels/jpeg_ops.hip``): raw planar frames in HBM -> complete
JFIF streams in HBM, one per batch row, which any decoder reads and an MJPG ``.avi`` stores as they
are.  Two launches, no host copy, no synchronisation, no allocation when the outputs and the
workspace are given: hipGraph-capturable.  The rule is all integer, so
:func:`~aiko_services_amd.ops.reference.jpeg_encode_ref` (the same in plain loops) equals the
kernels byte for byte.

**Input.**  One frame is the tightly packed planar ``i420`` or ``i444`` layout of
:func:`~aiko_services_amd.ops.yuv.frame_bytes`, full range: what ``rgb_to_yuv(..., standard="jpeg")``
writes, chroma centre-sited as in JPEG.  ``1 <= H <= 65535`` (the frame header's 16 bits), ``1 <= W <=
4096``, odd sizes legal.  An MCU (minimum coded unit) is 16 x 16 luma for ``i420`` (blocks Y00 Y01
Y10 Y11 Cb Cr) and 8 x 8 for ``i444`` (Y Cb Cr); ``mx = ceil(W / mcu_w)``, ``my = ceil(H / mcu_h)``.
A sample outside a component's plane is the plane's sample at the clamped coordinates.

**Forward DCT, integers only.**  :data:`DCT_MATRIX` ``M[k][n] = round(8192 * a_k * cos((2n+1) k pi /
16))``, ``a_0 = sqrt(1/8)``, ``a_k = 1/2`` (``M[0][0] = 2896``, ``M[1][0] = 4017``).  ``x = sample -
128``; columns first, ``t = (M @ x + 1024) >> 11``, then rows, ``c = (t @ M^T + 16384) >> 15``; the
shifts arithmetic, everything within int32.  Integer sums are order-free, so any summation order
gives the same bits (the kernel folds ``x[n] +- x[7-n]`` first: ``M[k][7-n] = (-1)^k M[k][n]``
exactly); a butterfly factorisation with intermediate roundings would not, and is not the rule.

**Quantisation.**  The Annex K tables (:data:`BASE_LUMA`, :data:`BASE_CHROMA`) scaled as libjpeg
does: ``s = 5000 // quality`` below 50, else ``200 - 2 * quality``; ``q = clamp((base * s + 50) //
100, 1, 255)``.  ``v = sign(c) * ((|c| + (q >> 1)) // q)``, clamped to ``[-1023, 1023]``.

**Entropy coding.**  The four typical Huffman tables of Annex K (:data:`HUFFMAN`), baseline coding
in :data:`ZIGZAG` order: the DC difference per component, the predictors 0 at the start of every
restart interval; run/size symbols, ``ZRL`` (0xF0) for every 16 zeros of a run, ``EOB`` (0x00) unless
coefficient 63 is non-zero; a negative value as ``v + (1 << size) - 1``.  Bits are packed MSB first,
a ``0xFF`` byte is followed by ``0x00``, a segment is padded to a byte with 1-bits.  The restart
interval is one MCU row (``DRI = mx``, also when ``my == 1``); ``RSTm``, ``m = row mod 8``, follows
every row's segment but the last.

**Stream.**  ``SOI``; ``APP0`` JFIF 1.01, units 0, density 1 x 1, no thumbnail; ``DQT`` 0 then ``DQT``
1 (8 bit, zigzag order, one segment each); ``SOF0`` (precision 8, H, W, components ``1: 0x22 | 0x11,
tq 0``, ``2: 0x11, tq 1``, ``3: 0x11, tq 1``); ``DHT`` 0x00, 0x10, 0x01, 0x11, one segment each;
``DRI``; ``SOS`` (components 1/0x00, 2/0x11, 3/0x11, then ``00 3F 00``); the segments and ``RST``
markers; ``EOI``.  Everything up to the first segment depends on ``(fmt, H, W, quality)`` only:
:func:`header` builds it on the host once and the kernel copies it.

**Output and capacity.**  ``stream`` uint8 ``[B, cap]``, ``nbytes`` int32 ``[B]``.  Frame ``b``
overflows iff its whole stream is longer than ``cap`` or any restart segment's stuffed length
(without its marker) exceeds ``seg_cap``.  Then ``nbytes[b] = -1`` and the row's contents are
unspecified; otherwise ``stream[b, :nbytes[b]]`` is the stream and the bytes at and past
``nbytes[b]`` are not written.  The other frames are unaffected either way.  The defaults
(:func:`capacities`): ``cap = len(header) + frame_bytes(fmt, H, W)``, ``seg_cap = frame_bytes(fmt,
mcu_h, W)``, at most 96 KiB, so a segment is built in LDS.

The device copies of the tables (:func:`device_tables`: the Huffman codes, the quantisers and their
reciprocals, the zigzag map and the header, one tensor) are uploaded at the first call for a
``(fmt, H, W, quality, device)`` and kept; call once before capturing a graph.
"""
from __future__ import annotations

import math
import struct
from functools import lru_cache

import torch

from .yuv import FORMATS, frame_bytes

__all__ = ["BASE_CHROMA", "BASE_LUMA", "DCT_MATRIX", "HUFFMAN", "JPEG_FORMATS", "MAX_HEIGHT", "MAX_SEG_CAP",
           "MAX_WIDTH", "TABLE_INTS", "ZIGZAG", "capacities", "device_tables", "geometry", "header",
           "huffman_codes", "jpeg_encode", "quant_tables", "workspace_bytes"]

#: format -> (MCU height, MCU width, blocks per MCU)
JPEG_FORMATS = {"i420": (16, 16, 6), "i444": (8, 8, 3)}
MAX_WIDTH = 4096
MAX_HEIGHT = 65535
MAX_SEG_CAP = 96 * 1024

#: ``DCT_MATRIX[k][n]``; the kernel holds a copy (``JP_DCT``) that a test pins equal
DCT_MATRIX = tuple(tuple(int(round(8192 * (math.sqrt(1 / 8) if k == 0 else 0.5) * math.cos((2 * n + 1) * k * math.pi / 16)))
                         for n in range(8)) for k in range(8))


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8 if (i // 8 + i % 8) % 2 else i % 8)))
    return tuple(order)


#: ``ZIGZAG[z]``: the natural (row-major) index of the coefficient at zigzag position ``z``
ZIGZAG = _zigzag()

#: the Annex K tables, natural order
BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

_AC_LUMA = ("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a34"
            "35363738393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a9293949596"
            "9798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1"
            "f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = ("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728"
              "292a35363738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92"
              "939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7"
              "e8e9eaf2f3f4f5f6f7f8f9fa")

#: DHT class/id byte -> (codes per length 1..16, the symbols in code order): Annex K's typical tables
HUFFMAN = {
    0x00: ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    0x10: ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), tuple(bytes.fromhex(_AC_LUMA))),
    0x01: ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    0x11: ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), tuple(bytes.fromhex(_AC_CHROMA))),
}

# the device table, in int32 units: Huffman entries are ``code | length << 16``
_T_AC, _T_DC, _T_Q, _T_RCP, _T_ZZ = 0, 512, 544, 672, 800
#: int32 entries in front of the header in :func:`device_tables`' tensor
TABLE_INTS = 864


def huffman_codes(table: int) -> dict:
    """symbol -> (code, length) of ``HUFFMAN[table]``: the canonical assignment of Annex C."""
    counts, symbols = HUFFMAN[table]
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _check_quality(quality) -> int:
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"jpeg: quality an integer in 1..100 required, got {quality!r}")
    return quality


def quant_tables(quality: int) -> tuple:
    """(luminance, chrominance) quantisers at ``quality``, 64 ints each, natural order."""
    quality = _check_quality(quality)
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(tuple(min(max((b * s + 50) // 100, 1), 255) for b in base) for base in (BASE_LUMA, BASE_CHROMA))


def geometry(fmt: str, height: int, width: int) -> tuple:
    """``(mcu_h, mcu_w, blocks per MCU, my, mx)``; ``ValueError`` for anything the coder does not take."""
    if fmt not in JPEG_FORMATS:
        raise ValueError(f"jpeg: format {fmt!r} cannot be coded (one of {sorted(JPEG_FORMATS)})")
    for v in (height, width):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"jpeg: height and width integers required, got {height!r} x {width!r}")
    h, w = int(height), int(width)
    if not (1 <= h <= MAX_HEIGHT and 1 <= w <= MAX_WIDTH):
        raise ValueError(f"jpeg: 1 <= height <= {MAX_HEIGHT} and 1 <= width <= {MAX_WIDTH} required, got {h} x {w}")
    mh, mw, nb = JPEG_FORMATS[fmt]
    return mh, mw, nb, -(-h // mh), -(-w // mw)


def _segment(marker: int, body: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


@lru_cache(maxsize=64)
def header(fmt: str, height: int, width: int, quality: int) -> bytes:
    """The stream from ``SOI`` to the end of ``SOS``."""
    mx = geometry(fmt, height, width)[4]
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    for tq, table in enumerate(quant_tables(quality)):
        out.append(_segment(0xDB, bytes([tq]) + bytes(table[n] for n in ZIGZAG)))
    luma = 0x22 if fmt == "i420" else 0x11
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, int(height), int(width), 3) +
                        bytes([1, luma, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc in (0x00, 0x10, 0x01, 0x11):
        counts, symbols = HUFFMAN[tc]
        out.append(_segment(0xC4, bytes([tc]) + bytes(counts) + bytes(symbols)))
    out.append(_segment(0xDD, struct.pack(">H", mx)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0])))
    return b"".join(out)


def capacities(fmt: str, height: int, width: int) -> tuple:
    """The default ``(cap, seg_cap)``: no stream of a frame is longer than the frame plus the header
    unless it is noise at the highest qualities."""
    mh = geometry(fmt, height, width)[0]
    return len(header(fmt, int(height), int(width), 90)) + frame_bytes(fmt, height, width), frame_bytes(fmt, mh, width)


def workspace_bytes(fmt: str, height: int, width: int, batch: int, seg_cap: int | None = None) -> int:
    """Bytes of the workspace of a call: per (frame, MCU row) an int32 length, then ``seg_cap`` bytes."""
    my = geometry(fmt, height, width)[3]
    seg_cap = capacities(fmt, height, width)[1] if seg_cap is None else int(seg_cap)
    return int(batch) * my * (4 + seg_cap)


def _table_ints(quality: int) -> list:
    ints = [0] * TABLE_INTS
    for tc, base in ((0x10, _T_AC), (0x11, _T_AC + 256), (0x00, _T_DC), (0x01, _T_DC + 16)):
        for symbol, (code, length) in huffman_codes(tc).items():
            ints[base + symbol] = code | length << 16
    for t, table in enumerate(quant_tables(quality)):
        for z, n in enumerate(ZIGZAG):
            q = table[n]
            ints[_T_Q + 64 * t + z] = q
            # (a * rcp) >> 32 == a // q for a < 2^16 and q >= 2; q == 1 has no 32-bit reciprocal: 0
            ints[_T_RCP + 64 * t + z] = (1 << 32) // q + 1 if q > 1 else 0
    for z, n in enumerate(ZIGZAG):
        ints[_T_ZZ + n] = z
    return ints


_DEVICE_TABLES = {}


def device_tables(fmt: str, height: int, width: int, quality: int, device) -> tuple:
    """``(tables, header length)``: uint8 on ``device``, :data:`TABLE_INTS` little-endian words (Huffman
    ``code | length << 16`` by symbol: AC luminance, AC chrominance at 256, DC at 512 and 528;
    quantisers in zigzag order at 544 and 608, their reciprocals at 672; natural index -> zigzag
    position at 800) and then the header.  Uploaded once per key."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (fmt, int(height), int(width), _check_quality(quality), device)
    hit = _DEVICE_TABLES.get(key)
    if hit is None:
        head = header(*key[:4])
        words = struct.pack(f"<{TABLE_INTS}I", *_table_ints(key[3]))
        if len(_DEVICE_TABLES) >= 64:
            _DEVICE_TABLES.pop(next(iter(_DEVICE_TABLES)))
        hit = _DEVICE_TABLES[key] = (torch.frombuffer(bytearray(words + head), dtype=torch.uint8).to(device), len(head))
    return hit


def jpeg_encode(raw: torch.Tensor, height: int, width: int, fmt: str = "i420", quality: int = 90, *,
                cap: int | None = None, seg_cap: int | None = None, stream: torch.Tensor | None = None,
                nbytes: torch.Tensor | None = None, workspace: torch.Tensor | None = None):
    """Device uint8 ``[B, frame_bytes(fmt, height, width)]`` -> ``(stream, nbytes)`` (the rule: this
    module's docstring).  ``cap`` defaults to ``stream``'s row length, else to :func:`capacities`';
    ``workspace`` is uint8, 4-byte aligned, of at least :func:`workspace_bytes` bytes.  Formats,
    qualities and shapes out of range are a ``ValueError``; dtypes, devices, contiguity and overlap are
    refused by the operator."""
    if fmt not in JPEG_FORMATS:
        raise ValueError(f"jpeg_encode: format {fmt!r} cannot be coded (one of {sorted(JPEG_FORMATS)})")
    _check_quality(quality)
    my = geometry(fmt, height, width)[3]
    need = frame_bytes(fmt, height, width)
    if raw.dim() != 2 or raw.shape[1] != need:
        raise ValueError(f"jpeg_encode: raw [B, {need}] required for {fmt} {height} x {width}, got {tuple(raw.shape)}")
    B = raw.shape[0]
    dcap, dseg = capacities(fmt, height, width)
    if cap is None:
        cap = stream.shape[1] if stream is not None and stream.dim() == 2 else dcap
    seg_cap = dseg if seg_cap is None else seg_cap
    for name, v, hi in (("cap", cap, 2 ** 31 - 1), ("seg_cap", seg_cap, MAX_SEG_CAP)):
        if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= hi:
            raise ValueError(f"jpeg_encode: {name} an integer in 1..{hi} required, got {v!r}")
    cap, seg_cap = int(cap), int(seg_cap)
    if stream is None:
        stream = torch.empty(B, cap, dtype=torch.uint8, device=raw.device)
    elif stream.dim() != 2 or tuple(stream.shape) != (B, cap):
        raise ValueError(f"jpeg_encode: stream [{B}, cap = {cap}] required, got {tuple(stream.shape)}")
    if nbytes is None:
        nbytes = torch.empty(B, dtype=torch.int32, device=raw.device)
    if workspace is None:
        workspace = torch.empty(B * my * (4 + seg_cap), dtype=torch.uint8, device=raw.device)
    tables, head = device_tables(fmt, height, width, quality, raw.device)
    torch.ops.aiko.jpeg_encode_out(raw, int(height), int(width), FORMATS[fmt], tables, head, seg_cap, stream, nbytes,
                                   workspace)
    return stream, nbytes
