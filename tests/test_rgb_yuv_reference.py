"""The torch reference of the YUV egress (``ops.reference.rgb_to_yuv_ref``): the table, every
(R, G, B) triple against the host converter, gray levels, output ranges and the round trip through
the decoder's reference; the chroma subsampling rule on crafted blocks and odd sizes; the four
layouts against each other; the Y4M writer's 4:2:0 and raw modes.  CPU only."""
import queue
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from aiko_services_amd.elements.media import video_io
from aiko_services_amd.ops.reference import rgb_to_yuv_ref, yuv_to_rgb_ref
from aiko_services_amd.ops.yuv import ENCODE_STANDARDS, FORMATS, STANDARDS, frame_bytes

N = 4096                       # 4096 x 4096 = 2^24 pixels: every triple once

_ALL = {}


def all_triples():
    """uint8 [1, N, N, 3] holding every (R, G, B) once (made once, never written)."""
    if "rgb" not in _ALL:
        r = torch.arange(256, dtype=torch.uint8)
        _ALL["rgb"] = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(1, N, N, 3).contiguous()
    return _ALL["rgb"]


def all_encoded(standard):
    """(Y, U, V) uint8 [N * N] each of every triple (computed once per standard)."""
    if standard not in _ALL:
        _ALL[standard] = rgb_to_yuv_ref(all_triples(), "i444", standard)
    return _ALL[standard][0].view(3, N * N)


def test_tables():
    assert sorted(ENCODE_STANDARDS) == ["bt601", "bt709", "jpeg"]
    assert ENCODE_STANDARDS["jpeg"] == (
        (0.0, 0.299, 0.587, 0.114, -0.168736, -0.331264, 0.5, 0.5, -0.418688, -0.081312), "half")
    assert ENCODE_STANDARDS["bt601"] == (
        (16.0, 0.256788, 0.504129, 0.097906, -0.148223, -0.290993, 0.439216, 0.439216, -0.367788, -0.071427), "rint")
    assert ENCODE_STANDARDS["bt709"] == (
        (16.0, 0.182586, 0.614231, 0.062007, -0.100644, -0.338572, 0.439216, 0.439216, -0.398942, -0.040274), "rint")
    for name, (_, rounding) in ENCODE_STANDARDS.items():
        assert rounding == STANDARDS[name][1]
    assert sorted(FORMATS) == ["i420", "i444", "nv12", "yuyv"]          # the encoder adds no layout


def test_jpeg_i444_equals_the_host_converter_on_every_triple():
    rgb = all_triples()
    y, u, v = video_io._rgb_to_yuv(rgb[0].numpy())
    got = all_encoded("jpeg")
    assert got.dtype == torch.uint8
    assert np.array_equal(got[0].numpy(), y.ravel())
    assert np.array_equal(got[1].numpy(), u.ravel())
    assert np.array_equal(got[2].numpy(), v.ravel())


@pytest.mark.parametrize("standard", ["jpeg", "bt601", "bt709"])
def test_gray_and_ranges(standard):
    level = torch.arange(256, dtype=torch.uint8)
    gray = level[None, None, :, None].expand(1, 1, 256, 3).contiguous()
    y, u, v = rgb_to_yuv_ref(gray, "i444", standard)[0].view(3, 256)
    assert (u == 128).all() and (v == 128).all()
    if standard == "jpeg":
        assert torch.equal(y, level)
    else:
        want = torch.round(16.0 + 219.0 * level.to(torch.float64) / 255.0).to(torch.uint8)
        assert torch.equal(y, want)
    y, u, v = all_encoded(standard)
    ranges = [(int(p.min()), int(p.max())) for p in (y, u, v)]
    print(standard, ranges)
    assert ranges == ([(0, 255), (1, 255), (1, 255)] if standard == "jpeg" else [(16, 235), (16, 240), (16, 240)])


@pytest.mark.parametrize("standard,bound", [("jpeg", 1), ("bt601", 2), ("bt709", 2)])
def test_round_trip_through_the_decoder(standard, bound):
    rgb = all_triples()
    all_encoded(standard)
    back = yuv_to_rgb_ref(_ALL[standard], N, N, "i444", standard)
    worst = int((back.to(torch.int16) - rgb.to(torch.int16)).abs().max())
    print(f"{standard}: worst round-trip difference {worst}")
    assert worst <= bound


# ---- the subsampling rule -------------------------------------------------------------------

def _sample(mean, row, rounding):
    """One chroma sample from a mean RGB triple, in the contract's order, as a Python int."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    x = ((f(row[0]) * f(mean[0]) + f(row[1]) * f(mean[1])) + f(row[2]) * f(mean[2])) + f(128.0)
    x = torch.round(x) if rounding == "rint" else torch.floor(x + 0.5)
    return int(x.clamp(0, 255))


def crafted_frame():
    """uint8 [1, 4, 6, 3]: block (0, 0) is (0, 0, 0, 1) per channel, block (0, 1) a block whose
    chroma-of-mean differs from the rounded mean of its pixels' chroma (found by search, bt601),
    the rest saturated colours."""
    if "crafted" not in _ALL:
        g = torch.Generator().manual_seed(11)
        found = None
        for _ in range(200):
            block = torch.randint(0, 256, (1, 2, 2, 3), dtype=torch.uint8, generator=g)
            per_pixel = rgb_to_yuv_ref(block, "i444", "bt601")[0].view(3, 4)[1:].to(torch.float64)
            of_mean = rgb_to_yuv_ref(block, "i420", "bt601")[0, 4:]
            mean_of = torch.floor(per_pixel.mean(1) + 0.5).to(torch.uint8)       # rounded mean of per-pixel chroma
            if not torch.equal(of_mean, mean_of):
                found = block
                break
        _ALL["crafted_block"] = found
        frame = torch.zeros(1, 4, 6, 3, dtype=torch.uint8)
        frame[0, 1, 1] = 1
        if found is not None:
            frame[0, 0:2, 2:4] = found[0]
        frame[0, 0:2, 4:6] = torch.tensor([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [255, 255, 255]]],
                                          dtype=torch.uint8)
        frame[0, 2:4] = torch.tensor([255, 0, 255], dtype=torch.uint8)
        frame[0, 3, 5] = torch.tensor([0, 255, 255], dtype=torch.uint8)
        _ALL["crafted"] = frame
    return _ALL["crafted"]


def test_quarter_mean_block():
    """(0, 0, 0, 1) per channel: mean 0.25, chroma from 0.25 and not from a rounded mean."""
    block = torch.zeros(1, 2, 2, 3, dtype=torch.uint8)
    block[0, 1, 1] = 1
    for standard, (coeffs, rounding) in ENCODE_STANDARDS.items():
        out = rgb_to_yuv_ref(block, "i420", standard)[0]
        assert out.shape == (6,)
        y = rgb_to_yuv_ref(block, "i444", standard)[0][:4]
        assert torch.equal(out[:4], y)
        assert int(out[4]) == _sample((0.25,) * 3, coeffs[4:7], rounding) == 128
        assert int(out[5]) == _sample((0.25,) * 3, coeffs[7:10], rounding) == 128
    # a coloured quarter: one pixel (255, 0, 0) of four, mean (63.75, 0, 0)
    block = torch.zeros(1, 2, 2, 3, dtype=torch.uint8)
    block[0, 0, 1, 0] = 255
    coeffs, rounding = ENCODE_STANDARDS["jpeg"]
    out = rgb_to_yuv_ref(block, "nv12", "jpeg")[0]
    assert int(out[4]) == _sample((63.75, 0.0, 0.0), coeffs[4:7], rounding) == 117
    assert int(out[5]) == _sample((63.75, 0.0, 0.0), coeffs[7:10], rounding) == 160


def test_chroma_of_mean_is_not_mean_of_chroma():
    crafted_frame()
    block = _ALL["crafted_block"]
    assert block is not None, "no 2x2 block among 200 random ones separates the two rules"
    coeffs, rounding = ENCODE_STANDARDS["bt601"]
    mean = [float(block[0, :, :, c].to(torch.int32).sum()) * 0.25 for c in range(3)]
    out = rgb_to_yuv_ref(block, "i420", "bt601")[0]
    assert int(out[4]) == _sample(mean, coeffs[4:7], rounding)
    assert int(out[5]) == _sample(mean, coeffs[7:10], rounding)
    per_pixel = rgb_to_yuv_ref(block, "i444", "bt601")[0].view(3, 4)[1:].to(torch.float64)
    assert not torch.equal(out[4:], torch.floor(per_pixel.mean(1) + 0.5).to(torch.uint8))


@pytest.mark.parametrize("h,w", [(5, 7), (6, 7), (5, 8), (1, 1)])
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_odd_sizes_use_edge_blocks(fmt, h, w):
    g = torch.Generator().manual_seed(100 * h + w)
    rgb = torch.randint(0, 256, (2, h, w, 3), dtype=torch.uint8, generator=g)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    for standard, (coeffs, rounding) in ENCODE_STANDARDS.items():
        out = rgb_to_yuv_ref(rgb, fmt, standard)
        assert tuple(out.shape) == (2, frame_bytes(fmt, h, w)) and out.dtype == torch.uint8
        assert torch.equal(out[:, :h * w], rgb_to_yuv_ref(rgb, "i444", standard)[:, :h * w])     # luma per pixel
        chroma = out[:, h * w:]
        if fmt == "nv12":
            u, v = chroma.view(2, ch, cw, 2)[..., 0], chroma.view(2, ch, cw, 2)[..., 1]
        else:
            u, v = chroma[:, :ch * cw].view(2, ch, cw), chroma[:, ch * cw:].view(2, ch, cw)
        for b in range(2):
            for cy in range(ch):
                for cx in range(cw):
                    px = rgb[b, 2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2].reshape(-1, 3).to(torch.int32)
                    n = px.shape[0]
                    assert n == (1 if 2 * cy + 1 == h else 2) * (1 if 2 * cx + 1 == w else 2)
                    mean = [float(px[:, c].sum()) * (1.0 / n) for c in range(3)]
                    assert int(u[b, cy, cx]) == _sample(mean, coeffs[4:7], rounding), (standard, b, cy, cx)
                    assert int(v[b, cy, cx]) == _sample(mean, coeffs[7:10], rounding), (standard, b, cy, cx)


def test_yuyv_uses_the_horizontal_pair():
    g = torch.Generator().manual_seed(9)
    rgb = torch.randint(0, 256, (2, 3, 6, 3), dtype=torch.uint8, generator=g)
    coeffs, rounding = ENCODE_STANDARDS["bt601"]
    out = rgb_to_yuv_ref(rgb, "yuyv", "bt601").view(2, 3, 3, 4)
    luma = rgb_to_yuv_ref(rgb, "i444", "bt601")[:, :18].view(2, 3, 6)
    assert torch.equal(out[..., 0], luma[..., 0::2]) and torch.equal(out[..., 2], luma[..., 1::2])
    for b in range(2):
        for y in range(3):
            for p in range(3):
                px = rgb[b, y, 2 * p:2 * p + 2].to(torch.int32)
                mean = [float(px[:, c].sum()) * 0.5 for c in range(3)]
                assert int(out[b, y, p, 1]) == _sample(mean, coeffs[4:7], rounding)
                assert int(out[b, y, p, 3]) == _sample(mean, coeffs[7:10], rounding)
    with pytest.raises(ValueError, match="even width"):
        rgb_to_yuv_ref(rgb[:, :, :5].contiguous(), "yuyv", "bt601")
    with pytest.raises(ValueError):
        rgb_to_yuv_ref(rgb, "p010", "bt601")
    with pytest.raises(ValueError):
        rgb_to_yuv_ref(rgb[..., :2].contiguous(), "nv12", "bt601")


def test_formats_agree_on_constant_blocks():
    """A picture whose 2x2 blocks are constant: the mean of a block is its colour, so nv12, i420
    and yuyv carry i444's samples at the block corners, in their own byte orders."""
    g = torch.Generator().manual_seed(2)
    B, H, W = 2, 6, 8
    small = torch.randint(0, 256, (B, H // 2, W // 2, 3), dtype=torch.uint8, generator=g)
    rgb = small.repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous()
    for std in ENCODE_STANDARDS:
        y, u, v = rgb_to_yuv_ref(rgb, "i444", std).view(B, 3, H, W).unbind(1)
        us, vs = u[:, 0::2, 0::2], v[:, 0::2, 0::2]
        flat = lambda *ps: torch.cat([p.reshape(B, -1) for p in ps], 1)  # noqa: E731
        assert torch.equal(rgb_to_yuv_ref(rgb, "i420", std), flat(y, us, vs))
        assert torch.equal(rgb_to_yuv_ref(rgb, "nv12", std), flat(y, torch.stack([us, vs], -1)))
        yuyv = torch.stack([y[..., 0::2], u[..., 0::2], y[..., 1::2], v[..., 0::2]], -1).reshape(B, -1)
        assert torch.equal(rgb_to_yuv_ref(rgb, "yuyv", std), yuyv)
        # and the decoder's reference gives the same picture back from all four
        back = yuv_to_rgb_ref(flat(y, u, v), H, W, "i444", std)
        for fmt in ("nv12", "i420", "yuyv"):
            assert torch.equal(yuv_to_rgb_ref(rgb_to_yuv_ref(rgb, fmt, std), H, W, fmt, std), back)


# ---- Y4M ------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(6, 10), (5, 7), (1, 1)])
def test_host_420_writer_equals_reference(tmp_path, h, w):
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
    frames.append(crafted_frame()[0].numpy()[:h, :w] if h <= 4 else frames[0][::-1].copy())
    path = tmp_path / "c420.y4m"
    wr = video_io.Y4MWriter(path, w, h, 25, chroma="420jpeg")
    for fr in frames:
        wr.write(fr)
    wr.close()
    assert path.read_bytes().split(b"\n", 1)[0] == f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420jpeg".encode()
    raw = list(video_io.iter_y4m(path, raw=True))
    assert len(raw) == len(frames)
    for fr, (fmt, hh, ww, packed) in zip(frames, raw):
        assert (fmt, hh, ww) == ("i420", h, w)
        want = rgb_to_yuv_ref(torch.from_numpy(fr.copy())[None], "i420", "jpeg")[0].numpy()
        assert np.array_equal(packed, want)


def test_write_raw_round_trip_and_headers(tmp_path):
    h, w = 5, 7
    g = torch.Generator().manual_seed(8)
    rgb = torch.randint(0, 256, (3, h, w, 3), dtype=torch.uint8, generator=g)
    for fmt, chroma, tag in (("i420", "420jpeg", b"C420jpeg"), ("i444", "444", b"C444")):
        frames = rgb_to_yuv_ref(rgb, fmt, "jpeg").numpy()
        path = tmp_path / f"{fmt}.y4m"
        wr = video_io.Y4MWriter(path, w, h, 30, chroma=chroma)
        for fr in frames:
            wr.write_raw(fr)
        with pytest.raises(ValueError, match="bytes"):
            wr.write_raw(frames[0][:-1])
        with pytest.raises(ValueError, match="bytes"):
            wr.write_raw(np.zeros(frame_bytes(fmt, h, w) + 1, np.uint8))
        wr.close()
        assert path.read_bytes().split(b"\n", 1)[0].split()[-1] == tag
        back = list(video_io.iter_y4m(path, raw=True))
        assert len(back) == 3                                            # the refused frames wrote nothing
        for fr, (f2, hh, ww, packed) in zip(frames, back):
            assert (f2, hh, ww) == (fmt, h, w) and np.array_equal(packed, fr)
    assert video_io.Y4MWriter.__init__.__defaults__[-1] == "444"        # the default stays C444
    with pytest.raises(ValueError, match="chroma"):
        video_io.Y4MWriter(tmp_path / "x.y4m", w, h, 30, chroma="422")


def _writer_element(target, **parameters):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    d = {"version": 0, "name": "p_write", "runtime": "python", "graph": ["(VideoWriteFile)"], "parameters": {},
         "elements": [{"name": "VideoWriteFile", "input": [{"name": "images", "type": "[image]"}], "output": [],
                       "parameters": {"data_targets": f"file://{target}", **parameters},
                       "deploy": {"local": {"module": "aiko_services_amd.elements.media.video_io"}}}]}
    p = PipelineImpl.create_pipeline("<write>", parse_pipeline_definition_dict(d), None, None, "w", [], 0, None, 60,
                                     queue_response=queue.Queue())
    element = p.pipeline_graph.get_node("VideoWriteFile").element
    stream = SimpleNamespace(variables={}, frame_id=0)
    event, _ = element.start_stream(stream, "w")
    assert event == 0
    return element, stream


def test_video_write_file_raw(tmp_path):
    from aiko_services_amd.pipeline.stream import StreamEvent
    h, w = 5, 7
    g = torch.Generator().manual_seed(12)
    rgb = torch.randint(0, 256, (2, h, w, 3), dtype=torch.uint8, generator=g)
    frames = rgb_to_yuv_ref(rgb, "i420", "jpeg").numpy()
    path = tmp_path / "out.y4m"
    element, stream = _writer_element(path, raw=True, format="i420", height=h, width=w, rate=25)
    assert element.process_frame(stream, images=[frames[0]])[0] == StreamEvent.OKAY
    assert element.process_frame(stream, images=[frames[1]])[0] == StreamEvent.OKAY
    event, out = element.process_frame(stream, images=[frames[1][:-1]])
    assert event == StreamEvent.ERROR and "bytes" in out["diagnostic"]
    element.stop_stream(stream, "w")
    back = list(video_io.iter_y4m(path, raw=True))
    assert [b[:3] for b in back] == [("i420", h, w)] * 2
    assert all(np.array_equal(b[3], f) for b, f in zip(back, frames))
    for target, parameters, match in [
            (tmp_path / "out.avi", dict(raw=True, format="i420", height=h, width=w), "y4m"),
            (tmp_path / "a.y4m", dict(raw=True, format="nv12", height=h, width=w), "format"),
            (tmp_path / "b.y4m", dict(raw=True, height=h, width=w), "format"),
            (tmp_path / "c.y4m", dict(raw=True, format="i444", width=w), "height and width"),
            (tmp_path / "d.y4m", dict(raw=True, format="i444", height=h), "height and width")]:
        element, stream = _writer_element(target, **parameters)
        event, out = element.process_frame(stream, images=[frames[0]])
        assert event == StreamEvent.ERROR and match in out["diagnostic"], (parameters, out)
        assert not target.exists()
