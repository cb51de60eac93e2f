"""Raw YUV frames -> uint8 RGB on the device (``csrc/kernels/yuv_ops.hip``): the output of a
hardware decoder (``nv12``), a camera (``yuyv``) or a Y4M file (``i420`` / ``i444``) becomes the
``[B, H, W, 3]`` batch every other op reads, without a host pass.  One launch, no synchronisation,
no allocation when ``out`` is given: hipGraph-capturable.

Frames are tightly packed; a row pitch or padded planes are out of scope.  With
``cw = (W+1)//2`` and ``ch = (H+1)//2``:

    nv12   Y plane H*W, then ch rows of cw interleaved (U, V) pairs       H*W + 2*ch*cw bytes
    i420   Y plane, U plane ch*cw, V plane ch*cw (Y4M ``C420*`` order)     H*W + 2*ch*cw
    i444   Y, U, V planes of H*W each (Y4M ``C444``)                      3*H*W
    yuyv   Y0 U Y1 V per pixel pair, W even                               2*H*W

Chroma is replicated, never interpolated: pixel (y, x) uses chroma sample (y//2, x//2), or
(y, x//2) for ``yuyv``.  Odd H and W are legal for the planar formats.

The arithmetic, in fp32, in exactly this order, no operation fused with another::

    c = (Y - yoff) * ygain;  u = U - 128;  v = V - 128
    r = c + rv*v;   g = (c - gu*u) - gv*v;   b = c + bu*u
    "rint": rint(x) (ties to even), then clamp to [0, 255]
    "half": x + 0.5, clamp to [0, 255], truncate

:data:`STANDARDS` is the one table of constants: the kernel takes them as arguments and
:func:`~aiko_services_amd.ops.reference.yuv_to_rgb_ref` reads the same rows.
"""
from __future__ import annotations

import torch

__all__ = ["BYTE_PIXELS", "ENCODE_STANDARDS", "FORMATS", "ROUND_MODES", "STANDARDS", "THREADS", "VECTOR_PIXELS",
           "encode_launch_grid", "encode_uses_vector", "frame_bytes", "launch_grid", "rgb_to_yuv", "unit_rows",
           "uses_vector", "yuv_to_rgb"]

#: format name -> the kernel's code
FORMATS = {"nv12": 0, "i420": 1, "i444": 2, "yuyv": 3}

#: rounding name -> the kernel's code
ROUND_MODES = {"rint": 0, "half": 1}

#: standard -> ((yoff, ygain, rv, gu, gv, bu), rounding).  ``bt601``: studio range, what
#: ``elements.media.v4l2.yuyv_to_rgb`` computes; ``jpeg``: full range, ``video_io._yuv_to_rgb``
#: (yoff 0 and ygain 1 leave Y as it is); ``bt709``: studio range, HD decoder output.
STANDARDS = {
    "bt601": ((16.0, 1.164383, 1.596027, 0.391762, 0.812968, 2.017232), "rint"),
    "jpeg": ((0.0, 1.0, 1.402, 0.344136, 0.714136, 1.772), "half"),
    "bt709": ((16.0, 1.164383, 1.792741, 0.213249, 0.532909, 2.112402), "rint"),
}

# the kernel's tiling (yuv_ops.hip: YUV_THREADS, YUV_VPX, YUV_BPX)
THREADS = 256            # threads of a workgroup
VECTOR_PIXELS = 16       # adjacent pixels a thread owns per row, vector kernel
BYTE_PIXELS = 2          # ... byte kernel


def frame_bytes(fmt: str, height: int, width: int) -> int:
    """Bytes of one tightly packed ``height`` x ``width`` frame."""
    if fmt not in FORMATS:
        raise ValueError(f"yuv: unknown format {fmt!r} (one of {sorted(FORMATS)})")
    h, w = int(height), int(width)
    if h < 1 or w < 1:
        raise ValueError(f"yuv: height and width >= 1 required, got {h} x {w}")
    if fmt == "i444":
        return 3 * h * w
    if fmt == "yuyv":
        if w % 2:
            raise ValueError(f"yuv: yuyv needs an even width, got {w}")
        return 2 * h * w
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def unit_rows(fmt: str) -> int:
    """Luma rows a thread owns: the two that share a chroma row for the 4:2:0 formats, else one."""
    return 2 if fmt in ("nv12", "i420") else 1


def uses_vector(raw: torch.Tensor, out: torch.Tensor, width: int) -> bool:
    """Whether the vector kernel serves this call: ``W % 16 == 0`` and both tensors 16-byte
    aligned (every plane and row offset of all four formats is then aligned for its load);
    every other call runs the byte kernel."""
    return int(width) % VECTOR_PIXELS == 0 and raw.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0


def launch_grid(fmt: str, height: int, width: int, batch: int, vector: bool) -> tuple[int, int]:
    """The launch's grid (workgroups per frame, frames) and, implicitly, its tail: a frame has
    ``ceil(H / unit_rows) * ceil(W / pixels per thread)`` threads in workgroups of THREADS."""
    px = VECTOR_PIXELS if vector else BYTE_PIXELS
    rows = unit_rows(fmt)
    units = ((int(height) + rows - 1) // rows) * ((int(width) + px - 1) // px)
    return (units + THREADS - 1) // THREADS, int(batch)


def yuv_to_rgb(raw: torch.Tensor, height: int, width: int, fmt: str = "nv12", standard: str = "bt601",
               out: torch.Tensor | None = None) -> torch.Tensor:
    """Device uint8 ``[B, frame_bytes(fmt, height, width)]`` (contiguous, frames tightly packed, no
    row pitch) -> ``out`` uint8 ``[B, height, width, 3]`` RGB by the ``standard``'s row of
    :data:`STANDARDS`.  ``out`` must not overlap ``raw``; by default it is new."""
    if fmt not in FORMATS:
        raise ValueError(f"yuv_to_rgb: unknown format {fmt!r} (one of {sorted(FORMATS)})")
    if standard not in STANDARDS:
        raise ValueError(f"yuv_to_rgb: unknown standard {standard!r} (one of {sorted(STANDARDS)})")
    coeffs, rounding = STANDARDS[standard]
    if out is None:
        nbytes = frame_bytes(fmt, height, width)
        if raw.dim() != 2 or raw.shape[1] != nbytes:
            raise ValueError(f"yuv_to_rgb: raw [B, {nbytes}] required for {fmt} {height} x {width}, "
                             f"got {tuple(raw.shape)}")
        out = torch.empty(raw.shape[0], int(height), int(width), 3, dtype=torch.uint8, device=raw.device)
    torch.ops.aiko.yuv_to_rgb_out(raw, int(height), int(width), FORMATS[fmt], list(coeffs), ROUND_MODES[rounding], out)
    return out


# ---- the way out: uint8 RGB -> raw frames (csrc/kernels/yuv_out_ops.hip) ----------------------
#
# The same layouts, written instead of read.  In fp32, in exactly this order, no operation fused
# with another:
#
#     y = ((yr*R + yg*G) + yb*B) + yoff
#     u = ((ur*Rm + ug*Gm) + ub*Bm) + 128
#     v = ((vr*Rm + vg*Gm) + vb*Bm) + 128
#     then the rounding of ROUND_MODES, as above
#
# R, G, B are the pixel's bytes; Rm, Gm, Bm the means over the in-frame pixels that share the
# chroma sample: the 2x2 block for nv12 / i420 (2 or 1 pixels at an odd right or bottom edge), the
# horizontal pair for yuyv, the pixel itself for i444.  The mean is the integer sum of the bytes,
# converted to float and multiplied by 1/n with n in {1, 2, 4}: both steps are exact.  Chroma is
# computed from the mean RGB, never averaged from per-pixel chroma: centre ("jpeg", MPEG-1)
# siting, the inverse of the decoder's chroma replication and what Y4M's ``C420jpeg`` names.

#: standard -> ((yoff, yr, yg, yb, ur, ug, ub, vr, vg, vb), rounding), the inverses of
#: :data:`STANDARDS`' rows.  ``jpeg`` is ``video_io._rgb_to_yuv`` bit for bit; ``bt601`` and
#: ``bt709`` map [0, 255] to studio range (Y in [16, 235], U and V in [16, 240]).
ENCODE_STANDARDS = {
    "jpeg": ((0.0, 0.299, 0.587, 0.114, -0.168736, -0.331264, 0.5, 0.5, -0.418688, -0.081312), "half"),
    "bt601": ((16.0, 0.256788, 0.504129, 0.097906, -0.148223, -0.290993, 0.439216, 0.439216, -0.367788, -0.071427),
              "rint"),
    "bt709": ((16.0, 0.182586, 0.614231, 0.062007, -0.100644, -0.338572, 0.439216, 0.439216, -0.398942, -0.040274),
              "rint"),
}


def encode_uses_vector(rgb: torch.Tensor, out: torch.Tensor) -> bool:
    """Whether the vector kernel serves this :func:`rgb_to_yuv` call: ``W % 16 == 0`` and both
    tensors 16-byte aligned (every plane, row and frame offset of all four formats is then aligned
    for its load or store); every other call runs the byte kernel."""
    return int(rgb.shape[2]) % VECTOR_PIXELS == 0 and rgb.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0


def encode_launch_grid(fmt: str, height: int, width: int, batch: int, vector: bool) -> tuple[int, int]:
    """The grid of an :func:`rgb_to_yuv` launch (workgroups per frame, frames): the tiling of
    yuv_out_ops.hip is that of the decoder (:func:`launch_grid`), a 4:2:0 thread owning both luma
    rows of its chroma row."""
    return launch_grid(fmt, height, width, batch, vector)


def rgb_to_yuv(rgb: torch.Tensor, fmt: str = "nv12", standard: str = "bt601",
               out: torch.Tensor | None = None) -> torch.Tensor:
    """Device uint8 ``[B, H, W, 3]`` RGB (contiguous) -> ``out`` uint8 ``[B, frame_bytes(fmt, H, W)]``,
    tightly packed frames, by the ``standard``'s row of :data:`ENCODE_STANDARDS`.  One launch, no
    synchronisation, no allocation when ``out`` is given.  ``out`` must not overlap ``rgb``; by
    default it is new."""
    if fmt not in FORMATS:
        raise ValueError(f"rgb_to_yuv: unknown format {fmt!r} (one of {sorted(FORMATS)})")
    if standard not in ENCODE_STANDARDS:
        raise ValueError(f"rgb_to_yuv: unknown standard {standard!r} (one of {sorted(ENCODE_STANDARDS)})")
    coeffs, rounding = ENCODE_STANDARDS[standard]
    if out is None:
        if rgb.dim() != 4 or rgb.shape[3] != 3:
            raise ValueError(f"rgb_to_yuv: rgb [B, H, W, 3] required, got {tuple(rgb.shape)}")
        nbytes = frame_bytes(fmt, rgb.shape[1], rgb.shape[2])           # yuyv with an odd width: ValueError
        out = torch.empty(rgb.shape[0], nbytes, dtype=torch.uint8, device=rgb.device)
    torch.ops.aiko.rgb_to_yuv_out(rgb, FORMATS[fmt], list(coeffs), ROUND_MODES[rounding], out)
    return out
