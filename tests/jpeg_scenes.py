"""Frames for the JPEG tests, CPU and GPU: raw planar ``i420`` / ``i444`` frames (the layout of
``ops.yuv.frame_bytes``) and their reference streams, computed once and shared.  A plain module: no
fixtures, no device."""
from __future__ import annotations

import io
from functools import lru_cache

import numpy as np
import torch

FORMATS = ("i420", "i444")
QUALITIES = (1, 50, 90, 100)
# the smallest shapes that can go wrong: one sample; one MCU of either format; partial MCUs right and
# bottom with odd chroma planes; more than 8 MCU rows (the RST counter wraps); more blocks in an MCU
# row than threads in a workgroup (270 for i420, 270 for i444: 9 passes, the last partial)
SHAPES = ((1, 1), (8, 8), (16, 16), (17, 23), (152, 24), (16, 720))
SUBSAMPLING = {"i420": 2, "i444": 0}                    # Pillow's name for each


def frame_bytes(fmt, H, W):
    from aiko_services_amd.ops.yuv import frame_bytes as fb
    return fb(fmt, H, W)


def structured_rgb(H: int, W: int, seed: int = 0) -> torch.Tensor:
    """uint8 ``[H, W, 3]``: smooth waves, a hard diagonal edge and a little noise."""
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(xx / 9.0 + yy / 23.0), 128 + 100 * np.cos(yy / 7.0), (xx * 3 + yy * 5) % 256], -1)
    base[(xx + 2 * yy) % 64 < 6] = 250
    noise = np.random.RandomState(seed).randn(H, W, 3) * 6
    return torch.from_numpy(np.clip(base + noise, 0, 255).astype(np.uint8))


def smooth_rgb(H: int, W: int) -> torch.Tensor:
    """uint8 ``[H, W, 3]``: gradients only, small at any quality."""
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([40 + 1.2 * xx + 0.3 * yy, 200 - 0.8 * yy, 90 + 0.5 * (xx + yy)], -1)
    return torch.from_numpy(np.clip(base, 0, 255).astype(np.uint8))


def smooth_noise_rgb(H: int, W: int, seed: int = 0) -> torch.Tensor:
    """uint8 ``[H, W, 3]``: the fidelity fixture, smooth gradients plus noise of sigma 10."""
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(xx / 9.0), 128 + 100 * np.cos(yy / 7.0), 40 + 2.5 * (xx + yy)], -1)
    noise = np.random.RandomState(seed).randn(H, W, 3) * 10
    return torch.from_numpy(np.clip(base + noise, 0, 255).astype(np.uint8))


def raw_from_rgb(rgb: torch.Tensor, fmt: str) -> torch.Tensor:
    """``[H, W, 3]`` or ``[B, H, W, 3]`` -> raw full-range frames ``[B, frame_bytes]``."""
    from aiko_services_amd.ops.reference import rgb_to_yuv_ref
    return rgb_to_yuv_ref(rgb if rgb.dim() == 4 else rgb[None], fmt, "jpeg")


def noise_raw(fmt: str, H: int, W: int, seed: int = 0, B: int = 1) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(0, 256, (B, frame_bytes(fmt, H, W)), dtype=torch.uint8, generator=g)


def flat_raw(fmt: str, H: int, W: int, yuv=(90, 120, 200)) -> torch.Tensor:
    ch, cw = ((H + 1) // 2, (W + 1) // 2) if fmt == "i420" else (H, W)
    return torch.cat([torch.full((n,), v, dtype=torch.uint8) for n, v in zip((H * W, ch * cw, ch * cw), yuv)])[None]


@lru_cache(maxsize=None)
def frames(fmt: str, H: int, W: int) -> torch.Tensor:
    """uint8 ``[3, frame_bytes]``: noise, flat, structured."""
    return torch.cat([noise_raw(fmt, H, W), flat_raw(fmt, H, W), raw_from_rgb(structured_rgb(H, W), fmt)])


def roomy(fmt: str, H: int, W: int) -> dict:
    """Capacities that noise at quality 100 fits: three times the defaults' payload, and room for the
    codes of a frame of a few samples, which are longer than the frame."""
    from aiko_services_amd.ops import jpeg as J
    cap, seg = J.capacities(fmt, H, W)
    return dict(cap=cap + 2 * frame_bytes(fmt, H, W) + 1024, seg_cap=min(3 * seg + 1024, J.MAX_SEG_CAP))


@lru_cache(maxsize=None)
def reference(fmt: str, H: int, W: int, quality: int):
    """``(stream, nbytes)`` of :func:`frames` at the capacities of :func:`roomy`."""
    from aiko_services_amd.ops.reference import jpeg_encode_ref
    return jpeg_encode_ref(frames(fmt, H, W), H, W, fmt, quality, **roomy(fmt, H, W))


def stream_bytes(stream: torch.Tensor, nbytes: torch.Tensor, b: int = 0) -> bytes:
    n = int(nbytes[b])
    assert n > 0, f"frame {b} overflowed"
    return bytes(stream[b, :n].cpu().tolist())


def decode(data: bytes) -> np.ndarray:
    """RGB uint8 ``[H, W, 3]`` by Pillow, fully loaded."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))


def pillow_encode(rgb: torch.Tensor, fmt: str, quality: int) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb.numpy(), "RGB").save(buf, format="JPEG", quality=quality, subsampling=SUBSAMPLING[fmt])
    return buf.getvalue()


def psnr(a, b) -> float:
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(10 * np.log10(255.0 ** 2 / max(float((d * d).mean()), 1e-12)))


def segments(data: bytes) -> list:
    """``(marker, body)`` of the marker segments in front of the entropy-coded data, SOS included."""
    assert data[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert data[i] == 0xFF, i
        marker, length = data[i + 1], data[i + 2] << 8 | data[i + 3]
        out.append((marker, data[i + 4:i + 2 + length]))
        i += 2 + length
        if marker == 0xDA:
            return out


def restart_markers(data: bytes, start: int) -> list:
    """The ``m`` of every ``RSTm`` in the entropy-coded data from ``start``."""
    return [data[i + 1] - 0xD0 for i in range(start, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


# ---- the cases a coder gets wrong -------------------------------------------------------------

# An 8 x 8 block whose only non-zero coefficient under the integer DCT is number 63, found by a
# search over perturbations of 128 + 110 cos((2r+1) 7 pi / 16) cos((2c+1) 7 pi / 16): at quality 100
# (every quantiser 1) it codes as DC 0, three ZRLs, the coefficient (440), and no EOB.
ONLY_63 = ((132, 116, 146, 107, 149, 110, 140, 124), (116, 162, 77, 188, 68, 179, 94, 140),
           (146, 77, 204, 38, 217, 52, 179, 110), (107, 188, 39, 234, 22, 218, 68, 149),
           (149, 68, 218, 22, 234, 38, 188, 107), (110, 179, 52, 218, 38, 204, 77, 146),
           (140, 94, 179, 68, 188, 77, 162, 116), (124, 140, 110, 149, 107, 146, 116, 132))


def only_63_raw() -> tuple:
    """``(raw, H, W, fmt)``: an i444 frame of one MCU, its Y block :data:`ONLY_63`, chroma flat."""
    y = torch.tensor(ONLY_63, dtype=torch.uint8).flatten()
    return torch.cat([y, torch.full((128,), 128, dtype=torch.uint8)])[None], 8, 8, "i444"


def checker_raw() -> tuple:
    """``(raw, H, W, fmt)``: a 0 / 255 checker of 8 x 8 squares in Y (i444, 16 x 40, chroma flat).  Left
    of x = 16 the squares sit on the block grid, so neighbouring blocks are all 0 and all 255 (DC
    difference 2039: size 11); from x = 16 on they are shifted by 4, so every block holds a 0 | 255
    step (an AC of size 10)."""
    H, W = 16, 40
    yy, xx = np.mgrid[0:H, 0:W]
    y = ((((xx + np.where(xx >= 16, 4, 0)) // 8 + yy // 8) % 2) * 255).astype(np.uint8)
    raw = torch.cat([torch.from_numpy(y).flatten(), torch.full((2 * H * W,), 128, dtype=torch.uint8)])
    return raw[None], H, W, "i444"


# ---- overflow -----------------------------------------------------------------------------------

OVERFLOW_SHAPE = (152, 24)


def one_noisy_row_raw() -> tuple:
    """``(raw, H, W, fmt)``: i420, flat but for the luma rows 32..47 (MCU row 2), which are noise."""
    H, W = OVERFLOW_SHAPE
    raw = flat_raw("i420", H, W).clone()
    g = torch.Generator().manual_seed(7)
    raw[0, 32 * W:48 * W] = torch.randint(0, 256, (16 * W,), dtype=torch.uint8, generator=g)
    return raw, H, W, "i420"
