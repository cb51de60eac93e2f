"""YUV egress on the MI355X (``yuv_out_ops.hip``): every (R, G, B) triple against the torch
reference bit for bit, the four layouts on vector and byte shapes, guard bands, hipGraph replay,
refusals, the round trip through the decoder, and the RgbToYuv / FrameDownload / VideoWriteFile
elements against the same kernel called directly."""
import json
import queue
from pathlib import Path

import numpy as np
import pytest
import torch

from kernel_guard import guarded

pytestmark = pytest.mark.gpu

FMTS = ["nv12", "i420", "i444", "yuyv"]
# one standard per layout in the geometry tests: both rounding modes and all three rows are used
STD_OF = {"nv12": "bt709", "i420": "jpeg", "i444": "bt709", "yuyv": "bt601"}
N = 4096                       # 4096 x 4096 = 2^24 pixels


# ---- every triple ---------------------------------------------------------------------------

_ALL = {}


def all_triples():
    """The frame holding every (R, G, B) once, [1, N, N, 3] on the host (made once)."""
    if "rgb" not in _ALL:
        r = torch.arange(256, dtype=torch.uint8)
        _ALL["rgb"] = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(1, N, N, 3).contiguous()
    return _ALL["rgb"]


def all_triples_ref(standard):
    if standard not in _ALL:
        from aiko_services_amd.ops.reference import rgb_to_yuv_ref
        _ALL[standard] = rgb_to_yuv_ref(all_triples(), "i444", standard)
    return _ALL[standard]


@pytest.mark.parametrize("standard", ["bt601", "jpeg", "bt709"])
@pytest.mark.parametrize("vector", [True, False])
def test_every_triple_equals_reference(native, standard, vector):
    """A product fused into its sum or a wrong rounding mode changes a few of the 2^24 triples:
    only the exhaustive frame sees them.  ``vector`` False: ``out`` starts one byte into a larger
    buffer, which only the byte kernel takes."""
    from aiko_services_amd.ops import yuv as Y
    rgb = all_triples().cuda()
    n = 3 * N * N
    buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    out = (buf[:n] if vector else buf[1:1 + n]).view(1, n)
    assert out.is_contiguous() and out.data_ptr() % 16 == (0 if vector else 1)
    assert Y.encode_uses_vector(rgb, out) == vector
    Y.rgb_to_yuv(rgb, "i444", standard, out=out)
    torch.cuda.synchronize()
    ref = all_triples_ref(standard)
    got = out.cpu()
    diff = int((got != ref).sum())
    print(f"{standard} vector={vector}: {diff} of {n} bytes differ")
    assert torch.equal(got, ref)


# ---- geometry -------------------------------------------------------------------------------

VECTOR_TAIL = (64, 144)        # 9 threads per row: waves span row ends; the last workgroup is partial
BYTE_TAIL = (21, 50)           # 25 threads per row, byte kernel: the last workgroup is partial
SMALL_SHAPES = [(1, 1), (5, 7), (6, 7), (5, 8), (2, 16), (3, 32), (7, 48)]


def test_tail_shapes_have_tails():
    from aiko_services_amd.ops import yuv as Y
    for fmt in FMTS:
        for (h, w), vector in ((VECTOR_TAIL, True), (BYTE_TAIL, False)):
            px = Y.VECTOR_PIXELS if vector else Y.BYTE_PIXELS
            units = -(-h // Y.unit_rows(fmt)) * -(-w // px)
            gx, gy = Y.encode_launch_grid(fmt, h, w, 3, vector)
            assert gx == -(-units // Y.THREADS) and gx >= 2 and gy == 3, (fmt, vector, gx, gy)
            assert units % Y.THREADS != 0, (fmt, vector, units)          # the last workgroup is partial
    assert VECTOR_TAIL[1] % Y.VECTOR_PIXELS == 0 and 64 % (VECTOR_TAIL[1] // Y.VECTOR_PIXELS) != 0


_CASES = {}


def crafted():
    """The crafted blocks of the CPU tests: the quarter-mean block, a block whose chroma-of-mean
    is not the rounded mean of its pixels' chroma, saturated colours; three frames of it."""
    from test_rgb_yuv_reference import crafted_frame
    return crafted_frame().expand(3, -1, -1, -1).contiguous()


def case(fmt, b, h, w):
    """(rgb, reference) on the host for seeded random pixels, computed once per case;
    ``h == "crafted"``: the crafted frame."""
    key = (fmt, b, h, w)
    if key not in _CASES:
        from aiko_services_amd.ops.reference import rgb_to_yuv_ref
        if h == "crafted":
            rgb = crafted()
        else:
            g = torch.Generator().manual_seed(1000 * h + w + b)
            rgb = torch.randint(0, 256, (b, h, w, 3), dtype=torch.uint8, generator=g)
        _CASES[key] = (rgb, rgb_to_yuv_ref(rgb, fmt, STD_OF[fmt]))
    return _CASES[key]


def misaligned(shape):
    """A contiguous device tensor one byte into a larger buffer, which only the byte kernel takes."""
    n = int(np.prod(shape))
    buf = torch.full((n + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + n].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 1
    return view


def _geometry_cases():
    cases = []
    for fmt in FMTS:
        for h, w in SMALL_SHAPES + [VECTOR_TAIL, BYTE_TAIL]:
            if fmt == "yuyv" and w % 2:
                continue                                  # odd widths: the planar layouts only
            cases.append((fmt, h, w, True))
            if w % 16 == 0:
                cases.append((fmt, h, w, False))          # a vector shape through the byte kernel
        cases.append((fmt, "crafted", 6, True))
    return cases


@pytest.mark.parametrize("fmt,h,w,aligned", _geometry_cases())
def test_equals_reference(native, fmt, h, w, aligned):
    from aiko_services_amd.ops import yuv as Y
    b = 3
    rgb, ref = case(fmt, b, h, w)
    h, w = rgb.shape[1:3]
    d = rgb.cuda()
    nbytes = Y.frame_bytes(fmt, h, w)
    out = torch.full((b, nbytes), 0x5A, dtype=torch.uint8, device="cuda") if aligned else misaligned((b, nbytes))
    vector = aligned and w % 16 == 0
    assert Y.encode_uses_vector(d, out) == vector        # which kernel runs follows from shape and alignment
    if aligned and (h, w) in (VECTOR_TAIL, BYTE_TAIL):
        assert vector == ((h, w) == VECTOR_TAIL)
        gx, _ = Y.encode_launch_grid(fmt, h, w, b, vector)
        px = Y.VECTOR_PIXELS if vector else Y.BYTE_PIXELS
        units = -(-h // Y.unit_rows(fmt)) * -(-w // px)
        assert gx >= 2 and units % Y.THREADS != 0        # the case really has a tail
    got = Y.rgb_to_yuv(d, fmt, STD_OF[fmt], out=out)
    torch.cuda.synchronize()
    assert got is out and torch.equal(out.cpu(), ref)
    assert torch.equal(d.cpu(), rgb)
    if aligned:                                          # the default output: new, same bytes
        fresh = Y.rgb_to_yuv(d, fmt, STD_OF[fmt])
        assert fresh.shape == (b, nbytes) and fresh.dtype == torch.uint8 and torch.equal(fresh.cpu(), ref)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("standard", ["bt601", "jpeg", "bt709"])
def test_crafted_blocks_every_standard(native, fmt, standard):
    from aiko_services_amd.ops import yuv as Y
    from aiko_services_amd.ops.reference import rgb_to_yuv_ref
    rgb = crafted()
    got = Y.rgb_to_yuv(rgb.cuda(), fmt, standard)
    assert torch.equal(got.cpu(), rgb_to_yuv_ref(rgb, fmt, standard))


def test_misaligned_input_takes_the_byte_kernel(native):
    from aiko_services_amd.ops import yuv as Y
    rgb, ref = case("nv12", 3, 7, 48)
    d = misaligned(rgb.shape)
    d.copy_(rgb)
    out = torch.empty(ref.shape, dtype=torch.uint8, device="cuda")
    assert not Y.encode_uses_vector(d, out)
    Y.rgb_to_yuv(d, "nv12", STD_OF["nv12"], out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)


# ---- guard bands ----------------------------------------------------------------------------

# every layout on one vector and one byte shape (odd sizes where the layout has them)
GUARD_CASES = [(fmt, (3, 7, 48), True) for fmt in FMTS] + \
    [(fmt, (3, 5, 8) if fmt == "yuyv" else (3, 5, 7), False) for fmt in FMTS]


@pytest.mark.parametrize("fmt,shape,vector", GUARD_CASES)
def test_guard_bands(native, fmt, shape, vector):
    from aiko_services_amd.ops import yuv as Y
    b, h, w = shape
    rgb, ref = case(fmt, b, h, w)
    fresh = Y.rgb_to_yuv(rgb.cuda(), fmt, STD_OF[fmt])
    gr, cr = guarded(rgb.shape, torch.uint8, "cuda", values=rgb, name="rgb")
    go, co = guarded(ref.shape, torch.uint8, "cuda", name="out")
    assert Y.encode_uses_vector(gr, go) == vector
    Y.rgb_to_yuv(gr, fmt, STD_OF[fmt], out=go)
    torch.cuda.synchronize()
    cr()
    co()
    assert torch.equal(gr.cpu(), rgb)                    # the input is unchanged
    # the output was all poison and the guards still are: equal to the run on fresh tensors (and
    # to the reference) means every byte was written, from bytes inside rgb
    assert torch.equal(go.cpu(), fresh.cpu()) and torch.equal(go.cpu(), ref)


# ---- hipGraph -------------------------------------------------------------------------------

def test_graph_replay_follows_the_input(native):
    from aiko_services_amd.ops import yuv as Y
    from aiko_services_amd.ops.reference import rgb_to_yuv_ref
    fmt, (b, h, w) = "nv12", (3, 7, 48)
    host, ref = case(fmt, b, h, w)
    rgb = host.cuda()
    buf = torch.empty(ref.shape, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Y.rgb_to_yuv(rgb, fmt, STD_OF[fmt], out=buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Y.rgb_to_yuv(rgb, fmt, STD_OF[fmt], out=buf)
    g = torch.Generator().manual_seed(77)
    other = torch.randint(0, 256, host.shape, dtype=torch.uint8, generator=g)
    other_ref = rgb_to_yuv_ref(other, fmt, STD_OF[fmt])
    assert not torch.equal(other_ref, ref)
    for src, want in ((host, ref), (other, other_ref), (host, ref)):
        rgb.copy_(src)
        buf.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf.cpu(), want)


# ---- refusals -------------------------------------------------------------------------------

def test_refusals(native):
    from aiko_services_amd.ops import yuv as Y
    from aiko_services_amd.ops.reference import rgb_to_yuv_ref
    b, h, w = 3, 7, 48
    host, ref = case("nv12", b, h, w)
    rgb = host.cuda()
    nbytes = ref.shape[1]
    out = torch.full((b, nbytes), 0x5A, dtype=torch.uint8, device="cuda")
    wide = torch.zeros(b, h, 2 * w, 3, dtype=torch.uint8, device="cuda")
    wide_out = torch.zeros(b, 2 * nbytes, dtype=torch.uint8, device="cuda")
    assert not wide[:, :, ::2].is_contiguous() and not wide_out[:, ::2].is_contiguous()
    odd = torch.zeros(b, 5, 7, 3, dtype=torch.uint8, device="cuda")

    def call(rgb=rgb, fmt="nv12", std="bt601", out=out):
        return Y.rgb_to_yuv(rgb, fmt, std, out=out)

    for match, kw in [
            ("rgb uint8", dict(rgb=rgb.view(torch.int8))),                   # not uint8
            ("rgb uint8", dict(rgb=rgb.float())),
            ("rgb uint8", dict(rgb=rgb.view(b, h * w, 3))),
            ("rgb uint8", dict(rgb=torch.zeros(b, h, w, 4, dtype=torch.uint8, device="cuda"))),
            ("contiguous", dict(rgb=wide[:, :, ::2])),
            ("out uint8", dict(out=out.view(torch.int8))),
            ("out uint8", dict(out=out.view(b, nbytes, 1))),
            ("out uint8", dict(out=torch.empty(b - 1, nbytes, dtype=torch.uint8, device="cuda"))),
            ("contiguous", dict(out=wide_out[:, ::2])),
            ("bytes", dict(out=torch.empty(b, nbytes - 1, dtype=torch.uint8, device="cuda"))),       # wrong out size
            ("bytes", dict(out=torch.empty(b, nbytes + 1, dtype=torch.uint8, device="cuda"))),
            ("bytes", dict(fmt="i444")),
            ("even width", dict(rgb=odd, fmt="yuyv", out=torch.empty(b, 70, dtype=torch.uint8, device="cuda"))),
            ("GPU tensor", dict(rgb=rgb.cpu())),
            ("GPU tensor", dict(out=torch.empty(b, nbytes, dtype=torch.uint8))),
            # all on the host: the dispatcher finds no kernel (the operator has none for the CPU)
            ("'CPU' backend", dict(rgb=rgb.cpu(), out=torch.empty(b, nbytes, dtype=torch.uint8)))]:
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    for match, kw in [("unknown format", dict(fmt="p010")), ("unknown standard", dict(std="bt2020")),
                      ("rgb \\[B, H, W, 3\\]", dict(rgb=rgb.view(b, h * w, 3), out=None)),
                      ("even width", dict(rgb=odd, fmt="yuyv", out=None))]:
        with pytest.raises(ValueError, match=match):
            call(**kw)
    # the operator itself: codes and coefficients
    coeffs = list(Y.ENCODE_STANDARDS["bt601"][0])
    op = torch.ops.aiko.rgb_to_yuv_out
    for match, args in [("unknown format", (rgb, 4, coeffs, 0, out)),
                        ("unknown format", (rgb, -1, coeffs, 0, out)),
                        ("unknown round mode", (rgb, 0, coeffs, 2, out)),
                        ("10 coefficients", (rgb, 0, coeffs[:9], 0, out)),
                        ("10 coefficients", (rgb, 0, coeffs + [1.0], 0, out)),
                        ("10 coefficients", (rgb, 0, list(Y.STANDARDS["bt601"][0]), 0, out)),       # the decoder's six
                        ("not finite", (rgb, 0, coeffs[:2] + [float("inf")] + coeffs[3:], 0, out)),
                        ("not finite", (rgb, 0, [float("nan")] + coeffs[1:], 0, out)),
                        ("not finite", (rgb, 0, coeffs[:9] + [1e39], 0, out))]:                     # inf as fp32
        with pytest.raises(RuntimeError, match=match):
            op(*args)
    # overlap: out starts inside rgb / rgb starts inside out; adjacent is fine
    nrgb = b * h * w * 3
    big = torch.zeros(nrgb + b * nbytes, dtype=torch.uint8, device="cuda")
    r = big[:nrgb].view(b, h, w, 3)
    with pytest.raises(RuntimeError, match="overlap"):
        call(rgb=r, out=big[nrgb - 1:nrgb - 1 + b * nbytes].view(b, nbytes))
    o = big[:b * nbytes].view(b, nbytes)
    with pytest.raises(RuntimeError, match="overlap"):
        call(rgb=big[b * nbytes - 1:b * nbytes - 1 + nrgb].view(b, h, w, 3), out=o)
    assert not big.any()
    r.copy_(rgb)
    adjacent = call(rgb=r, out=big[nrgb:].view(b, nbytes))
    with pytest.raises(RuntimeError, match="grid limit"):
        call(rgb=torch.zeros(65536, 1, 1, 3, dtype=torch.uint8, device="cuda"),
             out=torch.empty(65536, 3, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(adjacent.cpu(), rgb_to_yuv_ref(host, "nv12", "bt601"))
    assert (out == 0x5A).all()                           # no refused call wrote anything


# ---- round trip -----------------------------------------------------------------------------

def test_round_trip_on_the_device(native):
    from aiko_services_amd.ops import yuv as Y
    from aiko_services_amd.ops.reference import rgb_to_yuv_ref, yuv_to_rgb_ref
    b, h, w = 3, 6, 16
    g = torch.Generator().manual_seed(21)
    rgb = torch.randint(0, 256, (b, h, w, 3), dtype=torch.uint8, generator=g)
    raw = Y.rgb_to_yuv(rgb.cuda(), "nv12", "bt601")
    back = Y.yuv_to_rgb(raw, h, w, "nv12", "bt601")
    want_raw = rgb_to_yuv_ref(rgb, "nv12", "bt601")
    assert torch.equal(raw.cpu(), want_raw)
    assert torch.equal(back.cpu(), yuv_to_rgb_ref(want_raw, h, w, "nv12", "bt601"))


# ---- elements -------------------------------------------------------------------------------

VISION = "aiko_services_amd.elements.gpu.vision"
EGRESS = "aiko_services_amd.elements.gpu.egress"
VIDEO = "aiko_services_amd.elements.media.video_io"
EXAMPLES = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/yolo"


def _create(definition):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<rgb_yuv>", parse_pipeline_definition_dict(definition), None, None, "y", [], 0,
                                     None, 60, queue_response=q)
    return p, q


def _spy(element):
    """Clones of the ``images`` the element is given (its output replaces them in the swag)."""
    inner, seen = element.process_frame, []

    def spy(stream, images, *args, **kw):
        seen.append(images.clone())
        return inner(stream, images, *args, **kw)

    element.process_frame = spy
    return seen


def _element(name, module, inputs, outputs, parameters):
    return {"name": name, "input": [{"name": n, "type": "tensor"} for n in inputs],
            "output": [{"name": n, "type": t} for n, t in outputs], "parameters": parameters,
            "deploy": {"local": {"module": module}}}


@pytest.mark.parametrize("pool", [0, 2])
def test_rgb_to_yuv_element_equals_direct_call(native, pool):
    from aiko_services_amd.ops import yuv as Y
    from aiko_services_amd.ops.reference import rgb_to_yuv_ref
    b, h, w, frames = 2, 6, 48, 5
    d = {"version": 0, "name": "p_out", "runtime": "python", "graph": ["(SyntheticFrames RgbToYuv)"],
         "parameters": {"gpu_lanes": 2},
         "elements": [
             _element("SyntheticFrames", VISION, [], [("images", "tensor"), ("t_submit", "float")],
                      {"batch": b, "height": h, "width": w, "pool": 2, "stamp": True, "seed": 3}),
             _element("RgbToYuv", EGRESS, ["images"], [("images", "tensor")],
                      {"format": "nv12", "standard": "bt709", "pool": pool})]}
    p, q = _create(d)
    src = p.pipeline_graph.get_node("SyntheticFrames").element
    conv = p.pipeline_graph.get_node("RgbToYuv").element
    seen = _spy(conv)
    outs = []
    for i in range(frames):                              # more frames than slots: the slots recycle
        p.process_frame({"stream_id": "y", "frame_id": i}, {})
        info, out = q.get_nowait()
        assert info["state"] == 0, out
        torch.cuda.synchronize()
        outs.append(out["images"].clone())
    assert len(seen) == frames
    nbytes = Y.frame_bytes("nv12", h, w)
    for i, (rgb, raw) in enumerate(zip(seen, outs)):
        assert tuple(rgb.shape) == (b, h, w, 3)
        assert int(rgb.view(-1)[:8].cpu().view(torch.int64)) == i                   # the stamp: the frame id
        assert tuple(raw.shape) == (b, nbytes) and raw.dtype == torch.uint8 and raw.is_cuda
        assert torch.equal(raw, Y.rgb_to_yuv(rgb, "nv12", "bt709"))
        assert torch.equal(raw.cpu(), rgb_to_yuv_ref(rgb, "nv12", "bt709"))
    if pool:
        fp = conv._pools[(b, nbytes)]
        assert fp.capacity == 2 and fp.unheld_count() == 2                         # the slots came back
    else:
        assert not conv._pools and len(conv._out) >= 1
    assert src.frame_pool.unheld_count() == 2
    with pytest.raises(ValueError, match="images"):
        conv.process_frame(None, images=seen[0][0])


def test_frame_download_returns_the_device_bytes(native):
    d = {"version": 0, "name": "p_down", "runtime": "python", "graph": ["(SyntheticFrames FrameDownload)"],
         "parameters": {},
         "elements": [
             _element("SyntheticFrames", VISION, [], [("images", "tensor"), ("t_submit", "float")],
                      {"batch": 3, "height": 5, "width": 7, "pool": 2, "seed": 4}),
             _element("FrameDownload", EGRESS, ["images"], [("images", "[image]")], {})]}
    p, q = _create(d)
    down = p.pipeline_graph.get_node("FrameDownload").element
    seen = _spy(down)
    kept = []
    for i in range(6):                                   # more frames than the ring has sets
        p.process_frame({"stream_id": "y", "frame_id": i}, {})
        info, out = q.get_nowait()
        assert info["state"] == 0, out
        images = out["images"]
        assert isinstance(images, list) and len(images) == 3 and "format" not in out
        for j, frame in enumerate(images):
            assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.shape == (5, 7, 3)
            assert np.array_equal(frame, seen[i][j].cpu().numpy())
        kept.append((images, [f.copy() for f in images]))
    for images, copies in kept:                          # frames still held were not overwritten
        assert all(np.array_equal(a, c) for a, c in zip(images, copies))
    assert down.bytes_downloaded == 6 * 3 * 5 * 7 * 3
    # raw frames: the layout travels with them
    raw = torch.arange(2 * 64, dtype=torch.uint8, device="cuda").view(2, 64)          # i420 5 x 8: 40 + 2 * 12
    d["elements"][1]["parameters"] = {"format": "i420", "height": 5, "width": 8}
    d["elements"][1]["output"] += [{"name": n, "type": t} for n, t in
                                   (("format", "str"), ("height", "int"), ("width", "int"))]
    p2, _ = _create(d)
    down = p2.pipeline_graph.get_node("FrameDownload").element
    ev, out = down.process_frame(None, images=raw)
    assert ev == 0 and (out["format"], out["height"], out["width"]) == ("i420", 5, 8)
    assert [f.shape for f in out["images"]] == [(64,)] * 2
    assert np.array_equal(np.stack(out["images"]), raw.cpu().numpy())
    with pytest.raises(ValueError, match="raw i420"):
        down.process_frame(None, images=raw[:, :-1])
    with pytest.raises(ValueError, match="uint8"):
        down.process_frame(None, images=raw.float())


def test_device_frames_into_a_y4m_file(native, tmp_path):
    """RgbToYuv (i420, jpeg) -> FrameDownload -> VideoWriteFile with ``raw: true``: the file's
    frames are the reference's, and the file reads back as a picture."""
    from aiko_services_amd.elements.media import video_io
    from aiko_services_amd.ops.reference import rgb_to_yuv_ref, yuv_to_rgb_ref
    b, h, w, frames = 2, 5, 7, 3
    path = tmp_path / "out.y4m"
    d = {"version": 0, "name": "p_y4m", "runtime": "python",
         "graph": ["(SyntheticFrames RgbToYuv FrameDownload VideoWriteFile)"], "parameters": {},
         "elements": [
             _element("SyntheticFrames", VISION, [], [("images", "tensor"), ("t_submit", "float")],
                      {"batch": b, "height": h, "width": w, "pool": 2, "seed": 6}),
             _element("RgbToYuv", EGRESS, ["images"], [("images", "tensor")],
                      {"format": "i420", "standard": "jpeg"}),
             _element("FrameDownload", EGRESS, ["images"],
                      [("images", "[image]"), ("format", "str"), ("height", "int"), ("width", "int")],
                      {"format": "i420", "height": h, "width": w}),
             _element("VideoWriteFile", VIDEO, ["images"], [],
                      {"data_targets": f"file://{path}", "raw": True, "format": "i420", "height": h, "width": w,
                       "rate": 25})]}
    p, q = _create(d)
    seen = _spy(p.pipeline_graph.get_node("RgbToYuv").element)
    for i in range(frames):
        p.process_frame({"stream_id": "y", "frame_id": i}, {})
        info, out = q.get_nowait()
        assert info["state"] == 0, out
    writer = p.pipeline_graph.get_node("VideoWriteFile").element
    writer.stop_stream(p.stream_leases["y"].stream, "y")
    assert path.read_bytes().split(b"\n", 1)[0] == f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420jpeg".encode()
    want = torch.cat([rgb_to_yuv_ref(rgb, "i420", "jpeg") for rgb in seen])
    back = list(video_io.iter_y4m(path, raw=True))
    assert len(back) == frames * b and all(f[:3] == ("i420", h, w) for f in back)
    assert np.array_equal(np.stack([f[3] for f in back]), want.numpy())
    pictures = np.stack(list(video_io.iter_y4m(path)))
    assert np.array_equal(pictures, yuv_to_rgb_ref(want, h, w, "i420", "jpeg").numpy())


def test_example_pipeline_matches_direct_calls(native):
    from aiko_services_amd.models.yolov8 import YOLOv8
    from aiko_services_amd.ops import overlay as O
    from aiko_services_amd.ops import yuv as Y
    d = json.loads((EXAMPLES / "yolo_nv12_out_gpu.json").read_text())
    by_name = {e["name"]: e for e in d["elements"]}
    assert d["graph"] == ["(SyntheticFrames YuvToRgb YoloDetector DetectionOverlay RgbToYuv)"]
    assert by_name["SyntheticFrames"]["parameters"]["format"] == "nv12"
    assert by_name["RgbToYuv"]["parameters"]["format"] == "nv12"
    assert by_name["RgbToYuv"]["parameters"]["standard"] == by_name["YuvToRgb"]["parameters"]["standard"] == "bt601"
    by_name["SyntheticFrames"]["parameters"].update(batch=2)
    by_name["YoloDetector"]["parameters"].update(autotune=False, graph=True)
    p, q = _create(d)
    p.response_swag = True
    raws = _spy(p.pipeline_graph.get_node("YuvToRgb").element)
    overlay = p.pipeline_graph.get_node("DetectionOverlay").element
    yolo = YOLOv8(scale="n", seed=0, device="cuda", conf=0.25)
    nbytes = 480 * 640 * 3 // 2
    for i in range(3):
        p.process_frame({"stream_id": "y", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        torch.cuda.synchronize()
        raw = raws[i]
        assert tuple(raw.shape) == (2, nbytes) and tuple(swag["images"].shape) == (2, nbytes)
        rgb = Y.yuv_to_rgb(raw, 480, 640, "nv12", "bt601")
        det, count = yolo.detect(rgb)
        assert torch.equal(swag["detections"], det) and torch.equal(swag["counts"], count)
        names, font, palette, gw = overlay._ensure_tables(None)
        drawn = O.draw_detections(rgb, det, count, overlay.k, names, font, palette, thickness=overlay.thickness,
                                  text_scale=overlay.text_scale, margin=overlay.margin,
                                  show_score=overlay.show_score, glyph_width=gw)
        assert torch.equal(swag["images"], Y.rgb_to_yuv(drawn, "nv12", "bt601"))
