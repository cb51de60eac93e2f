"""YUV ingest on the MI355X (``yuv_ops.hip``): every (Y, U, V) triple against the torch reference
bit for bit, the four layouts on vector and byte shapes, guard bands, hipGraph replay, refusals,
and the SyntheticFrames / FrameUpload / YuvToRgb elements against the same kernel called directly."""
import json
import queue
from pathlib import Path

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
    """The i444 frame holding every (Y, U, V) once, [1, 3 * 2^24] on the host (made once)."""
    if "raw" not in _ALL:
        r = torch.arange(256, dtype=torch.uint8)
        y, u, v = torch.meshgrid(r, r, r, indexing="ij")
        _ALL["raw"] = torch.cat([y.reshape(-1), u.reshape(-1), v.reshape(-1)])[None].contiguous()
    return _ALL["raw"]


def all_triples_ref(standard):
    if standard not in _ALL:
        from aiko_services_amd.ops.reference import yuv_to_rgb_ref
        _ALL[standard] = yuv_to_rgb_ref(all_triples(), N, N, "i444", standard)
    return _ALL[standard]


@pytest.mark.parametrize("standard", ["bt601", "jpeg", "bt709"])
def test_every_triple_equals_reference(native, standard):
    """A fused multiply-add in g changes 26 (bt601) / 42 (jpeg) of the 2^24 triples, a wrong
    rounding mode every tie: only the exhaustive frame sees them."""
    from aiko_services_amd.ops import yuv as Y
    raw = all_triples().cuda()
    out = torch.empty(1, N, N, 3, dtype=torch.uint8, device="cuda")
    assert Y.uses_vector(raw, out, N)
    Y.yuv_to_rgb(raw, N, N, "i444", standard, out=out)
    torch.cuda.synchronize()
    ref = all_triples_ref(standard)
    got = out.cpu()
    diff = int((got != ref).any(-1).sum())
    print(f"{standard}: {diff} of {N * N} triples differ")
    assert torch.equal(got, ref)


def test_every_triple_byte_kernel(native):
    from aiko_services_amd.ops import yuv as Y
    n = 3 * N * N
    buf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    raw = buf[1:1 + n].view(1, n)
    raw.copy_(all_triples())
    out = torch.empty(1, N, N, 3, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 1 and raw.is_contiguous() and not Y.uses_vector(raw, out, N)
    Y.yuv_to_rgb(raw, N, N, "i444", "bt601", out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), all_triples_ref("bt601"))


# ---- geometry -------------------------------------------------------------------------------

def tile_shape():
    """(H, W) from the kernel's tile constants: more than two workgroups per frame and a partial
    last one for every layout, in the vector and in the byte kernel."""
    from aiko_services_amd.ops import yuv as Y
    groups = 5
    return 2 * (2 * Y.THREADS // groups + 2) - 1, groups * Y.VECTOR_PIXELS


def _units(fmt, h, w, vector):
    from aiko_services_amd.ops import yuv as Y
    px = Y.VECTOR_PIXELS if vector else Y.BYTE_PIXELS
    rows = Y.unit_rows(fmt)
    return -(-h // rows) * -(-w // px)


def test_tile_shape_spans_workgroups():
    from aiko_services_amd.ops import yuv as Y
    h, w = tile_shape()
    assert (h, w) == (207, 80) and h % 2 == 1 and w % Y.VECTOR_PIXELS == 0
    for fmt in FMTS:
        for vector in (True, False):
            units = _units(fmt, h, w, vector)
            gx, gy = Y.launch_grid(fmt, h, w, 3, vector)
            assert gx == -(-units // Y.THREADS) and gx >= 3 and gy == 3, (fmt, vector, gx, gy)
            assert units % Y.THREADS != 0, (fmt, vector, units)             # the last workgroup is partial


_CASES = {}


def case(fmt, b, h, w):
    """(raw, reference) on the host for seeded random bytes, computed once per case."""
    key = (fmt, b, h, w)
    if key not in _CASES:
        from aiko_services_amd.ops.reference import yuv_to_rgb_ref
        from aiko_services_amd.ops.yuv import frame_bytes
        g = torch.Generator().manual_seed(1000 * h + w + b)
        raw = torch.randint(0, 256, (b, frame_bytes(fmt, h, w)), dtype=torch.uint8, generator=g)
        _CASES[key] = (raw, yuv_to_rgb_ref(raw, h, w, fmt, STD_OF[fmt]))
    return _CASES[key]


def on_device(raw, aligned=True):
    """A contiguous device copy of ``raw``: from the allocator (256-byte aligned) or one byte into
    a larger buffer, which only the byte kernel takes."""
    if aligned:
        return raw.cuda()
    buf = torch.empty(raw.numel() + 16, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + raw.numel()].view(raw.shape)
    view.copy_(raw)
    assert view.is_contiguous() and view.data_ptr() % 16 == 1
    return view


VECTOR_SHAPES = [(3, 6, 48), (3, 5, 32), (1, 5, 32)]
BYTE_SHAPES = [(3, 5, 7), (3, 4, 6), (3, 3, 18), (1, 3, 18), (1, 5, 7)]


def _geometry_cases():
    cases = []
    for fmt in FMTS:
        for shape in VECTOR_SHAPES + ["tile"]:
            cases += [(fmt, shape, True, True), (fmt, shape, False, False)]
        for shape in BYTE_SHAPES:
            if fmt == "yuyv" and shape[2] % 2:
                continue                                  # odd widths: the planar layouts only
            cases.append((fmt, shape, True, False))
    return cases


@pytest.mark.parametrize("fmt,shape,aligned,vector", _geometry_cases())
def test_equals_reference(native, fmt, shape, aligned, vector):
    from aiko_services_amd.ops import yuv as Y
    b, h, w = (3, *tile_shape()) if shape == "tile" else shape
    raw, ref = case(fmt, b, h, w)
    d = on_device(raw, aligned)
    out = torch.full((b, h, w, 3), 0x5A, dtype=torch.uint8, device="cuda")
    assert Y.uses_vector(d, out, w) == vector            # which kernel runs follows from shape and alignment
    got = Y.yuv_to_rgb(d, h, w, fmt, STD_OF[fmt], out=out)
    torch.cuda.synchronize()
    assert got is out and torch.equal(out.cpu(), ref)
    assert torch.equal(d.cpu(), raw)
    if aligned:                                          # the default output: new, same bytes
        fresh = Y.yuv_to_rgb(d, h, w, fmt, STD_OF[fmt])
        assert fresh.shape == (b, h, w, 3) and fresh.dtype == torch.uint8 and torch.equal(fresh.cpu(), ref)


def test_misaligned_output_takes_the_byte_kernel(native):
    from aiko_services_amd.ops import yuv as Y
    raw, ref = case("nv12", 3, 6, 48)
    d = raw.cuda()
    buf = torch.empty(ref.numel() + 16, dtype=torch.uint8, device="cuda")
    out = buf[3:3 + ref.numel()].view(ref.shape)
    assert not Y.uses_vector(d, out, 48)
    Y.yuv_to_rgb(d, 6, 48, "nv12", STD_OF["nv12"], out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)


# ---- guard bands ----------------------------------------------------------------------------

# every layout on one vector and one byte shape (odd sizes where the layout has them)
GUARD_CASES = [(fmt, (3, 5, 32), True) for fmt in FMTS] + \
    [(fmt, (3, 4, 6) if fmt == "yuyv" else (3, 5, 7), False) for fmt in FMTS]


@pytest.mark.parametrize("fmt,shape,vector", GUARD_CASES)
def test_guard_bands(native, fmt, shape, vector):
    from aiko_services_amd.ops import yuv as Y
    b, h, w = shape
    raw, ref = case(fmt, b, h, w)
    fresh = Y.yuv_to_rgb(raw.cuda(), h, w, fmt, STD_OF[fmt])
    gr, cr = guarded(raw.shape, torch.uint8, "cuda", values=raw, name="raw")
    go, co = guarded((b, h, w, 3), torch.uint8, "cuda", name="out")
    assert Y.uses_vector(gr, go, w) == vector
    Y.yuv_to_rgb(gr, h, w, fmt, STD_OF[fmt], out=go)
    torch.cuda.synchronize()
    cr()
    co()
    assert torch.equal(gr.cpu(), raw)                    # the input is unchanged
    # the output was all poison and the guards still are: equal to the run on fresh tensors (and
    # to the reference) means every byte was written from bytes inside raw
    assert torch.equal(go.cpu(), fresh.cpu()) and torch.equal(go.cpu(), ref)


# ---- hipGraph -------------------------------------------------------------------------------

def test_graph_replay_follows_the_input(native):
    from aiko_services_amd.ops import yuv as Y
    from aiko_services_amd.ops.reference import yuv_to_rgb_ref
    fmt, (b, h, w) = "nv12", (3, 6, 48)
    host, ref = case(fmt, b, h, w)
    raw = host.cuda()
    buf = torch.empty(b, h, w, 3, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Y.yuv_to_rgb(raw, h, w, fmt, STD_OF[fmt], out=buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Y.yuv_to_rgb(raw, h, w, fmt, STD_OF[fmt], out=buf)
    g = torch.Generator().manual_seed(77)
    other = torch.randint(0, 256, host.shape, dtype=torch.uint8, generator=g)
    other_ref = yuv_to_rgb_ref(other, h, w, fmt, STD_OF[fmt])
    assert not torch.equal(other_ref, ref)
    for src, want in ((host, ref), (other, other_ref), (host, ref)):
        raw.copy_(src)
        buf.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf.cpu(), want)


# ---- refusals -------------------------------------------------------------------------------

def test_refusals(native):
    from aiko_services_amd.ops import yuv as Y
    from aiko_services_amd.ops.reference import yuv_to_rgb_ref
    b, h, w = 3, 6, 48
    host, _ = case("nv12", b, h, w)
    raw = host.cuda()
    out = torch.full((b, h, w, 3), 0x5A, dtype=torch.uint8, device="cuda")
    nbytes = raw.shape[1]
    wide = torch.zeros(b, 2 * nbytes, dtype=torch.uint8, device="cuda")
    assert not wide[:, ::2].is_contiguous()
    wide_out = torch.zeros(b, h, 2 * w, 3, dtype=torch.uint8, device="cuda")

    def call(raw=raw, h=h, w=w, fmt="nv12", std="bt601", out=out):
        return Y.yuv_to_rgb(raw, h, w, fmt, std, out=out)

    for match, kw in [
            ("bytes", dict(raw=raw[:, :-1].contiguous())),                   # wrong byte count
            ("bytes", dict(raw=torch.zeros(b, nbytes + 1, dtype=torch.uint8, device="cuda"))),
            ("bytes", dict(fmt="i444")),
            ("raw uint8", dict(raw=raw.view(b * nbytes))),
            ("raw uint8", dict(raw=raw.view(torch.int8))),
            ("raw uint8", dict(raw=raw.float())),
            ("contiguous", dict(raw=wide[:, ::2])),
            ("even width", dict(raw=torch.zeros(b, 2 * 5 * 7, dtype=torch.uint8, device="cuda"), h=5, w=7, fmt="yuyv",
                                out=torch.empty(b, 5, 7, 3, dtype=torch.uint8, device="cuda"))),
            ("out uint8", dict(out=torch.empty(b, h, w + 1, 3, dtype=torch.uint8, device="cuda"))),
            ("out uint8", dict(out=torch.empty(b - 1, h, w, 3, dtype=torch.uint8, device="cuda"))),
            ("out uint8", dict(out=torch.empty(b, h, w, 4, dtype=torch.uint8, device="cuda"))),
            ("out uint8", dict(out=torch.empty(b, h * w, 3, dtype=torch.uint8, device="cuda"))),
            ("out uint8", dict(out=torch.empty(b, h, w, 3, dtype=torch.int8, device="cuda"))),
            ("contiguous", dict(out=wide_out[:, :, ::2])),
            ("height, width", dict(h=0)),
            ("GPU tensor", dict(raw=raw.cpu())),
            ("GPU tensor", dict(out=torch.empty(b, h, w, 3, dtype=torch.uint8))),
            # all on the host: the dispatcher finds no kernel (the operator has none for the CPU)
            ("'CPU' backend", dict(raw=raw.cpu(), out=torch.empty(b, h, w, 3, dtype=torch.uint8)))]:
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    for match, kw in [("unknown format", dict(fmt="p010")), ("unknown standard", dict(std="bt2020")),
                      ("raw \\[B, ", dict(raw=raw[:, :-1].contiguous(), out=None)),
                      ("even width", dict(raw=raw, h=5, w=7, fmt="yuyv", out=None))]:
        with pytest.raises(ValueError, match=match):
            call(**kw)
    # the operator itself: codes and coefficients
    coeffs = list(Y.STANDARDS["bt601"][0])
    op = torch.ops.aiko.yuv_to_rgb_out
    for match, args in [("unknown format", (raw, h, w, 4, coeffs, 0, out)),
                        ("unknown format", (raw, h, w, -1, coeffs, 0, out)),
                        ("unknown round mode", (raw, h, w, 0, coeffs, 2, out)),
                        ("6 coefficients", (raw, h, w, 0, coeffs[:5], 0, out)),
                        ("6 coefficients", (raw, h, w, 0, coeffs + [1.0], 0, out)),
                        ("not finite", (raw, h, w, 0, coeffs[:2] + [float("inf")] + coeffs[3:], 0, out)),
                        ("not finite", (raw, h, w, 0, [float("nan")] + coeffs[1:], 0, out)),
                        ("not finite", (raw, h, w, 0, coeffs[:5] + [1e39], 0, out))]:     # inf as fp32
        with pytest.raises(RuntimeError, match=match):
            op(*args)
    # overlap: out starts inside raw / raw starts inside out; adjacent is fine
    big = torch.zeros(b * nbytes + b * h * w * 3, dtype=torch.uint8, device="cuda")
    r = big[:b * nbytes].view(b, nbytes)
    with pytest.raises(RuntimeError, match="overlap"):
        call(raw=r, out=big[b * nbytes - 1:b * nbytes - 1 + b * h * w * 3].view(b, h, w, 3))
    o = big[:b * h * w * 3].view(b, h, w, 3)
    with pytest.raises(RuntimeError, match="overlap"):
        call(raw=big[b * h * w * 3 - 1:b * h * w * 3 - 1 + b * nbytes].view(b, nbytes), out=o)
    assert not big.any()
    r.copy_(raw)
    adjacent = call(raw=r, out=big[b * nbytes:].view(b, h, w, 3))
    with pytest.raises(RuntimeError, match="grid limit"):
        call(raw=torch.zeros(65536, 3, dtype=torch.uint8, device="cuda"), h=1, w=1,
             out=torch.empty(65536, 1, 1, 3, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(adjacent.cpu(), yuv_to_rgb_ref(host, h, w, "nv12", "bt601"))
    assert (out == 0x5A).all()                           # no refused call wrote anything


# ---- elements -------------------------------------------------------------------------------

VISION = "aiko_services_amd.elements.gpu.vision"
INGEST = "aiko_services_amd.elements.gpu.ingest"
EXAMPLES = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/yolo"


def _create(definition):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<yuv>", parse_pipeline_definition_dict(definition), None, None, "y", [], 0,
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


def test_synthetic_nv12_into_yuv_to_rgb(native):
    from aiko_services_amd.ops import yuv as Y
    from aiko_services_amd.ops.reference import yuv_to_rgb_ref
    b, h, w, frames = 2, 6, 48, 5
    d = {"version": 0, "name": "p_nv12", "runtime": "python", "graph": ["(SyntheticFrames YuvToRgb)"],
         "parameters": {"gpu_lanes": 2},
         "elements": [
             _element("SyntheticFrames", VISION, [], [("images", "tensor"), ("t_submit", "float")],
                      {"batch": b, "height": h, "width": w, "pool": 2, "format": "nv12", "stamp": True, "seed": 3}),
             _element("YuvToRgb", INGEST, ["images"], [("images", "tensor")],
                      {"format": "nv12", "standard": "bt709", "height": h, "width": w, "pool": 2})]}
    p, q = _create(d)
    src = p.pipeline_graph.get_node("SyntheticFrames").element
    conv = p.pipeline_graph.get_node("YuvToRgb").element
    seen = _spy(conv)
    outs = []
    for i in range(frames):                              # more frames than slots: the slots recycle
        p.process_frame({"stream_id": "y", "frame_id": i}, {})
        info, out = q.get_nowait()
        assert info["state"] == 0, out
        torch.cuda.synchronize()
        outs.append(out["images"].clone())
    assert p.share["gpu_lanes"] == 2 and len(seen) == frames
    nbytes = Y.frame_bytes("nv12", h, w)
    for i, (raw, rgb) in enumerate(zip(seen, outs)):
        assert tuple(raw.shape) == (b, nbytes) and raw.dtype == torch.uint8 and raw.is_cuda
        assert int(raw.view(-1)[:8].cpu().view(torch.int64)) == i                   # the stamp: the frame id
        assert torch.equal(raw.view(-1)[8:], seen[0].view(-1)[8:])
        assert tuple(rgb.shape) == (b, h, w, 3)
        assert torch.equal(rgb, Y.yuv_to_rgb(raw, h, w, "nv12", "bt709"))
        assert torch.equal(rgb.cpu(), yuv_to_rgb_ref(raw, h, w, "nv12", "bt709"))
    pool = conv._pools[b]
    assert pool.capacity == 2 and pool.unheld_count() == 2                         # the slots came back
    assert src.frame_pool.unheld_count() == 2
    with pytest.raises(ValueError, match="bytes"):
        conv.process_frame(None, images=seen[0][:, :-1])


def test_host_yuyv_upload_then_convert(native):
    from aiko_services_amd.ops import yuv as Y
    from aiko_services_amd.ops.reference import yuv_to_rgb_ref
    b, h, w, frames = 3, 4, 6, 4
    d = {"version": 0, "name": "p_yuyv", "runtime": "python", "graph": ["(SyntheticFrames FrameUpload YuvToRgb)"],
         "parameters": {},
         "elements": [
             _element("SyntheticFrames", VISION, [], [("images", "tensor"), ("t_submit", "float")],
                      {"batch": b, "height": h, "width": w, "pool": 3, "format": "yuyv", "host": True, "seed": 5}),
             _element("FrameUpload", VISION, ["images"], [("images", "tensor")],
                      {"pool": 4, "format": "yuyv", "height": h, "width": w}),
             _element("YuvToRgb", INGEST, ["images"], [("images", "tensor")],
                      {"format": "yuyv", "standard": "bt601", "height": h, "width": w})]}
    p, q = _create(d)
    src = p.pipeline_graph.get_node("SyntheticFrames").element
    up = p.pipeline_graph.get_node("FrameUpload").element
    for i in range(frames):
        p.process_frame({"stream_id": "y", "frame_id": i}, {})
        info, out = q.get_nowait()
        assert info["state"] == 0, out
        torch.cuda.synchronize()
        host = src.host_pool[i % 3]
        assert tuple(host.shape) == (b, 2 * h * w)
        assert torch.equal(out["images"].cpu(), yuv_to_rgb_ref(host, h, w, "yuyv", "bt601")), i
    assert up.bytes_uploaded == frames * b * 2 * h * w                              # two thirds of RGB's
    assert up.bytes_uploaded * 3 == 2 * (frames * b * h * w * 3)
    # the other raw inputs: a numpy batch, a list of arrays, a list of bytes
    host = src.host_pool[0]
    want = yuv_to_rgb_ref(host, h, w, "yuyv", "bt601")
    for images in (host.numpy(), [row.numpy() for row in host], [row.numpy().tobytes() for row in host]):
        ev, out = up.process_frame(None, images=images)
        assert ev == 0 and tuple(out["images"].shape) == (b, 2 * h * w)
        assert torch.equal(Y.yuv_to_rgb(out["images"], h, w, "yuyv", "bt601").cpu(), want)
    with pytest.raises(ValueError, match="raw yuyv"):
        up.process_frame(None, images=torch.zeros(b, h, w, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="raw yuyv"):
        up.process_frame(None, images=[bytes(2 * h * w - 1)])


def test_example_pipeline_matches_direct_call(native):
    from aiko_services_amd.models.yolov8 import YOLOv8
    from aiko_services_amd.ops import yuv as Y
    d = json.loads((EXAMPLES / "yolo_nv12_gpu.json").read_text())
    by_name = {e["name"]: e for e in d["elements"]}
    assert d["graph"] == ["(SyntheticFrames YuvToRgb YoloDetector DetectionOverlay)"]
    assert by_name["SyntheticFrames"]["parameters"]["format"] == "nv12"
    assert (by_name["YuvToRgb"]["parameters"]["height"], by_name["YuvToRgb"]["parameters"]["width"]) == (480, 640)
    by_name["SyntheticFrames"]["parameters"].update(batch=2)
    by_name["YoloDetector"]["parameters"].update(autotune=False, graph=True)
    p, q = _create(d)
    p.response_swag = True
    raws = _spy(p.pipeline_graph.get_node("YuvToRgb").element)
    rgbs = _spy(p.pipeline_graph.get_node("YoloDetector").element)
    yolo = YOLOv8(scale="n", seed=0, device="cuda", conf=0.25)
    for i in range(3):
        p.process_frame({"stream_id": "y", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        torch.cuda.synchronize()
        raw, rgb = raws[i], rgbs[i]
        assert tuple(raw.shape) == (2, 480 * 640 * 3 // 2) and tuple(rgb.shape) == (2, 480, 640, 3)
        assert torch.equal(rgb, Y.yuv_to_rgb(raw, 480, 640, "nv12", "bt601"))       # the detector's input
        det, count = yolo.detect(rgb)
        assert torch.equal(swag["detections"], det) and torch.equal(swag["counts"], count)
        assert tuple(swag["images"].shape) == (2, 480, 640, 3)
