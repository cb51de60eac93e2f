"""The torch reference of the YUV ingest (``ops.reference.yuv_to_rgb_ref``) against the host
converters it replaces, bit for bit over all 2^24 (Y, U, V) triples; frame sizes; the raw output of
the Y4M reader and the camera's byte accounting.  CPU only."""
import numpy as np
import pytest
import torch

from aiko_services_amd.elements.media import v4l2, video_io
from aiko_services_amd.ops.reference import yuv_to_rgb_ref
from aiko_services_amd.ops.yuv import FORMATS, STANDARDS, frame_bytes

N = 4096                       # 4096 x 4096 = 2^24 pixels: every triple once


def test_tables():
    assert sorted(FORMATS) == ["i420", "i444", "nv12", "yuyv"] and sorted(FORMATS.values()) == [0, 1, 2, 3]
    assert sorted(STANDARDS) == ["bt601", "bt709", "jpeg"]
    assert STANDARDS["bt601"] == ((16.0, 1.164383, 1.596027, 0.391762, 0.812968, 2.017232), "rint")
    assert STANDARDS["jpeg"] == ((0.0, 1.0, 1.402, 0.344136, 0.714136, 1.772), "half")
    assert STANDARDS["bt709"] == ((16.0, 1.164383, 1.792741, 0.213249, 0.532909, 2.112402), "rint")


def test_jpeg_i444_equals_the_y4m_converter_on_every_triple():
    y, u, v = (p.reshape(N, N) for p in np.meshgrid(*[np.arange(256, dtype=np.uint8)] * 3, indexing="ij"))
    want = video_io._yuv_to_rgb(y, u, v)
    raw = torch.from_numpy(np.concatenate([y.ravel(), u.ravel(), v.ravel()]))[None]
    got = yuv_to_rgb_ref(raw, N, N, "i444", "jpeg")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, N, N, 3)
    assert np.array_equal(got[0].numpy(), want)


def test_bt601_yuyv_equals_the_camera_converter_on_every_triple():
    # per (U, V) 128 pixel pairs (Y0, Y1) = (2p, 2p + 1): 2^16 * 128 pairs of 4 bytes
    u, v, p = np.meshgrid(*[np.arange(256, dtype=np.uint8)] * 2, np.arange(128, dtype=np.uint8), indexing="ij")
    buf = np.stack([2 * p, u, 2 * p + 1, v], -1).astype(np.uint8).reshape(-1)
    assert buf.size == 2 * N * N == frame_bytes("yuyv", N, N)
    want = v4l2.yuyv_to_rgb(buf, N, N)
    got = yuv_to_rgb_ref(torch.from_numpy(buf)[None], N, N, "yuyv", "bt601")
    assert np.array_equal(got[0].numpy(), want)


def test_frame_bytes():
    assert frame_bytes("nv12", 480, 640) == frame_bytes("i420", 480, 640) == 480 * 640 * 3 // 2
    assert frame_bytes("i444", 480, 640) == 480 * 640 * 3
    assert frame_bytes("yuyv", 480, 640) == 480 * 640 * 2
    assert frame_bytes("nv12", 5, 7) == frame_bytes("i420", 5, 7) == 35 + 2 * 3 * 4
    assert frame_bytes("i420", 5, 8) == 40 + 2 * 3 * 4 and frame_bytes("i420", 6, 7) == 42 + 2 * 3 * 4
    assert frame_bytes("i444", 5, 7) == 105
    assert frame_bytes("yuyv", 5, 6) == 60
    assert frame_bytes("nv12", 1, 1) == 3
    with pytest.raises(ValueError, match="even width"):
        frame_bytes("yuyv", 5, 7)
    with pytest.raises(ValueError, match="unknown format"):
        frame_bytes("p010", 4, 4)
    with pytest.raises(ValueError):
        frame_bytes("nv12", 0, 4)


def test_formats_agree_on_replicated_chroma():
    """The same picture in all four layouts: 4:2:0 chroma written out per pixel for i444, per
    pixel pair and row for yuyv."""
    g = torch.Generator().manual_seed(2)
    B, H, W = 2, 6, 8
    y = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, generator=g)
    u = torch.randint(0, 256, (B, H // 2, W // 2), dtype=torch.uint8, generator=g)
    v = torch.randint(0, 256, (B, H // 2, W // 2), dtype=torch.uint8, generator=g)
    up = lambda p: p.repeat_interleave(2, 1).repeat_interleave(2, 2)  # noqa: E731
    flat = lambda *ps: torch.cat([p.reshape(B, -1) for p in ps], 1)  # noqa: E731
    i420 = flat(y, u, v)
    nv12 = flat(y, torch.stack([u, v], -1))
    i444 = flat(y, up(u), up(v))
    yuyv = torch.stack([y[..., 0::2], up(u)[..., 0::2], y[..., 1::2], up(v)[..., 0::2]], -1).reshape(B, -1)
    for std in STANDARDS:
        ref = yuv_to_rgb_ref(i420, H, W, "i420", std)
        assert torch.equal(yuv_to_rgb_ref(nv12, H, W, "nv12", std), ref)
        assert torch.equal(yuv_to_rgb_ref(i444, H, W, "i444", std), ref)
        assert torch.equal(yuv_to_rgb_ref(yuyv, H, W, "yuyv", std), ref)
    assert not torch.equal(yuv_to_rgb_ref(i420, H, W, "i420", "bt601"), yuv_to_rgb_ref(i420, H, W, "i420", "bt709"))
    with pytest.raises(ValueError):
        yuv_to_rgb_ref(i420[:, :-1], H, W, "i420", "bt601")


def test_y4m_c444_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, (6, 10, 3), dtype=np.uint8) for _ in range(3)]
    path = tmp_path / "c444.y4m"
    video_io.write_y4m(path, frames)
    rgb = list(video_io.iter_y4m(path))
    raw = list(video_io.iter_y4m(path, raw=True))
    assert len(rgb) == len(raw) == 3
    for want, (fmt, h, w, packed) in zip(rgb, raw):
        assert (fmt, h, w) == ("i444", 6, 10)
        assert packed.dtype == np.uint8 and packed.shape == (frame_bytes("i444", 6, 10),)
        got = yuv_to_rgb_ref(torch.from_numpy(packed.copy())[None], h, w, fmt, "jpeg")
        assert np.array_equal(got[0].numpy(), want)
    assert [p.shape for p in video_io.iter_video_frames(path, raw=True)] == [(180,)] * 3


def test_y4m_c420_odd_sizes(tmp_path):
    h, w, ch, cw = 5, 7, 3, 4
    rng = np.random.default_rng(5)
    planes = [rng.integers(0, 256, h * w + 2 * ch * cw, dtype=np.uint8) for _ in range(2)]
    path = tmp_path / "c420.y4m"
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{w} H{h} F30:1 Ip A1:1 C420jpeg\n".encode())
        for p in planes:
            f.write(b"FRAME\n" + p.tobytes())
    rgb = list(video_io.iter_y4m(path))
    raw = list(video_io.iter_y4m(path, raw=True))
    assert len(rgb) == len(raw) == 2
    for want, plane, (fmt, hh, ww, packed) in zip(rgb, planes, raw):
        assert (fmt, hh, ww) == ("i420", h, w) and np.array_equal(packed, plane)
        got = yuv_to_rgb_ref(torch.from_numpy(packed.copy())[None], h, w, "i420", "jpeg")
        assert want.shape == (h, w, 3) and np.array_equal(got[0].numpy(), want)


def test_raw_refusals(tmp_path):
    path = tmp_path / "c422.y4m"
    path.write_bytes(b"YUV4MPEG2 W4 H2 F30:1 Ip A1:1 C422\nFRAME\n" + bytes(16))
    with pytest.raises(ValueError, match="C422"):
        next(video_io.iter_y4m(path, raw=True))
    other = tmp_path / "frames.npy"
    np.save(other, np.zeros((1, 2, 2, 3), np.uint8))
    assert len(list(video_io.iter_video_frames(other))) == 1
    with pytest.raises(ValueError, match="y4m"):
        next(video_io.iter_video_frames(other, raw=True))


def test_camera_buffer_byte_accounting():
    """``V4L2Capture.read(raw=True)`` hands out the first 2*W*H bytes of the mmap'd buffer as a 1-D
    copy; no device here, so the same slice of a buffer (longer than the frame, as the driver's
    page-rounded ones are) goes through the host converter and the reference."""
    w, h = 6, 4
    rng = np.random.default_rng(6)
    buf = rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    raw = np.frombuffer(buf, dtype=np.uint8, count=w * h * 2).copy()
    assert raw.shape == (frame_bytes("yuyv", h, w),) and raw.size * 3 == 2 * (h * w * 3)
    want = v4l2.yuyv_to_rgb(buf, w, h)
    got = yuv_to_rgb_ref(torch.from_numpy(raw)[None], h, w, "yuyv", "bt601")
    assert np.array_equal(got[0].numpy(), want)
