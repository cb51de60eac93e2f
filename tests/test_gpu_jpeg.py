"""The JPEG kernels (``ops.jpeg.jpeg_encode``, jpeg_ops.hip) against the CPU reference, byte for byte,
on the frames of jpeg_scenes.py; the cases a coder gets wrong, the overflow rule, guard bands, graph
replay and refusals; then the elements against direct calls and the example pipeline end to end."""
import json
import queue
from pathlib import Path

import pytest
import torch

import jpeg_scenes as S
from kernel_guard import guarded

pytestmark = pytest.mark.gpu


def _ref(raw, H, W, fmt, quality, **kw):
    from aiko_services_amd.ops.reference import jpeg_encode_ref
    return jpeg_encode_ref(raw, H, W, fmt, quality, **kw)


def _assert_streams(got, want, where):
    """``nbytes`` equal, and every frame that did not overflow equal in its ``nbytes`` bytes."""
    (gs, gn), (ws, wn) = got, want
    gs, gn = gs.cpu(), gn.cpu()
    assert gn.dtype == torch.int32 and gs.dtype == torch.uint8 and gs.shape == ws.shape, where
    assert torch.equal(gn, wn), f"{where}: nbytes {gn.tolist()} != {wn.tolist()}"
    for b, n in enumerate(wn.tolist()):
        if n > 0 and not torch.equal(gs[b, :n], ws[b, :n]):
            first = int(torch.nonzero(gs[b, :n] != ws[b, :n])[0])
            raise AssertionError(f"{where}: frame {b} differs first at byte {first} of {n}")


@pytest.mark.parametrize("fmt", S.FORMATS)
@pytest.mark.parametrize("H,W", S.SHAPES)
def test_streams_equal_reference(native, fmt, H, W):
    from aiko_services_amd.ops.jpeg import jpeg_encode
    raw = S.frames(fmt, H, W).cuda()
    for quality in S.QUALITIES:
        want = S.reference(fmt, H, W, quality)
        assert int(want[1].min()) > 0                      # nothing overflows at these capacities
        got = jpeg_encode(raw, H, W, fmt, quality, **S.roomy(fmt, H, W))
        torch.cuda.synchronize()
        _assert_streams(got, want, f"{fmt} {H} x {W} quality {quality}")


def test_widest_frame(native):
    """W = 4096: 1536 blocks in an MCU row, and a bitstream past 64 KiB of LDS."""
    from aiko_services_amd.ops import jpeg as J
    H, W, fmt = 16, 4096, "i420"
    cap, seg_cap = J.capacities(fmt, H, W)
    assert seg_cap == J.MAX_SEG_CAP
    raw = torch.cat([S.noise_raw(fmt, H, W), S.raw_from_rgb(S.structured_rgb(H, W), fmt)])
    want = _ref(raw, H, W, fmt, 75, cap=2 * cap)
    assert int(want[1].min()) > 0 and int(want[1].max()) > 32 * 1024
    got = J.jpeg_encode(raw.cuda(), H, W, fmt, 75, cap=2 * cap)
    torch.cuda.synchronize()
    _assert_streams(got, want, "16 x 4096")


@pytest.mark.parametrize("scene", [S.only_63_raw, S.checker_raw])
def test_pinned_coder_cases(native, scene):
    """Three ZRLs and no EOB; a DC difference of size 11 and an AC of size 10 (that the scenes hold
    them: test_jpeg_reference.py)."""
    from aiko_services_amd.ops.jpeg import jpeg_encode
    raw, H, W, fmt = scene()
    want = _ref(raw, H, W, fmt, 100, cap=8192, seg_cap=4096)
    assert int(want[1][0]) > 0
    got = jpeg_encode(raw.cuda(), H, W, fmt, 100, cap=8192, seg_cap=4096)
    torch.cuda.synchronize()
    _assert_streams(got, want, scene.__name__)


def test_overflow_leaves_neighbours_exact(native):
    from aiko_services_amd.ops import jpeg as J
    H, W = S.OVERFLOW_SHAPE
    fmt = "i420"
    cap, seg_cap = J.capacities(fmt, H, W)
    noisy_row = S.one_noisy_row_raw()[0]
    raw = torch.cat([S.flat_raw(fmt, H, W), S.noise_raw(fmt, H, W), S.raw_from_rgb(S.smooth_rgb(H, W), fmt),
                     noisy_row])
    # quality 100, defaults: the noise is past cap (and seg_cap), the noisy row past seg_cap only
    want = _ref(raw, H, W, fmt, 100)
    assert want[1].tolist()[1] == -1 and want[1].tolist()[3] == -1 and min(want[1].tolist()[::2]) > 0
    stream = torch.full((4, cap), 0x5A, dtype=torch.uint8, device="cuda")
    got = J.jpeg_encode(raw.cuda(), H, W, fmt, 100, stream=stream)
    torch.cuda.synchronize()
    _assert_streams(got, want, "defaults")
    for b in (0, 2):                                       # bytes at and past nbytes are not written
        assert bool((got[0][b, int(got[1][b]):] == 0x5A).all())
    # cap alone: roomy segments, the noise still past the default cap, the noisy row now fits
    want = _ref(raw, H, W, fmt, 100, seg_cap=4 * seg_cap)
    assert want[1].tolist()[1] == -1 and want[1].tolist()[3] > 0
    got = J.jpeg_encode(raw.cuda(), H, W, fmt, 100, seg_cap=4 * seg_cap)
    torch.cuda.synchronize()
    _assert_streams(got, want, "roomy segments")
    # the boundaries: exactly the stream's length fits, one byte less does not
    exact = int(want[1][3])
    for c, fits in ((exact, True), (exact - 1, False)):
        got = J.jpeg_encode(raw[3:].cuda(), H, W, fmt, 100, cap=c, seg_cap=4 * seg_cap)
        torch.cuda.synchronize()
        assert int(got[1][0]) == (exact if fits else -1)
    # quality 90: everything fits the defaults
    want = _ref(raw, H, W, fmt, 90)
    assert int(want[1].min()) > 0
    _assert_streams(J.jpeg_encode(raw.cuda(), H, W, fmt, 90), want, "quality 90")


@pytest.mark.parametrize("fmt,H,W", [("i420", 17, 23), ("i444", 152, 24), ("i420", 16, 720)])
def test_guard_bands_and_poison_past_nbytes(native, fmt, H, W):
    from aiko_services_amd.ops import jpeg as J
    raw = S.frames(fmt, H, W)
    kw = S.roomy(fmt, H, W)
    want = S.reference(fmt, H, W, 90)
    checks = []

    def g(shape, dtype, values=None, name=""):
        view, check = guarded(shape, dtype, "cuda", values=values, name=name)
        checks.append(check)
        return view

    graw = g(raw.shape, torch.uint8, raw, "raw")
    stream, nbytes = g((3, kw["cap"]), torch.uint8, name="stream"), g((3,), torch.int32, name="nbytes")
    workspace = g((J.workspace_bytes(fmt, H, W, 3, kw["seg_cap"]),), torch.uint8, name="workspace")
    tables, head = J.device_tables(fmt, H, W, 90, "cuda")
    gtab = g(tables.shape, torch.uint8, tables, "tables")
    torch.ops.aiko.jpeg_encode_out(graw, H, W, {"i420": 1, "i444": 2}[fmt], gtab, head, kw["seg_cap"], stream, nbytes,
                                   workspace)
    torch.cuda.synchronize()
    for check in checks:
        check()
    _assert_streams((stream, nbytes), want, "guarded")
    for b in range(3):                                     # bytes at and past nbytes keep their poison
        assert bool((stream[b, int(nbytes[b]):] == 0xA5).all())
    assert torch.equal(graw.cpu(), raw) and torch.equal(gtab, tables)
    plain = J.jpeg_encode(raw.cuda(), H, W, fmt, 90, **kw)
    torch.cuda.synchronize()
    _assert_streams(plain, want, "unguarded")


def test_two_batches_through_one_graph(native):
    from aiko_services_amd.ops import jpeg as J
    fmt, H, W = "i420", 40, 56
    kw = S.roomy(fmt, H, W)
    batches = [S.frames(fmt, H, W), torch.cat([S.raw_from_rgb(S.smooth_noise_rgb(H, W, s), fmt) for s in range(3)])]
    wants = [_ref(b, H, W, fmt, 75, **kw) for b in batches]
    raw = torch.empty_like(batches[0], device="cuda")
    stream = torch.empty(3, kw["cap"], dtype=torch.uint8, device="cuda")
    nbytes = torch.empty(3, dtype=torch.int32, device="cuda")
    workspace = torch.empty(J.workspace_bytes(fmt, H, W, 3, kw["seg_cap"]), dtype=torch.uint8, device="cuda")

    def run():
        J.jpeg_encode(raw, H, W, fmt, 75, seg_cap=kw["seg_cap"], stream=stream, nbytes=nbytes, workspace=workspace)

    raw.copy_(batches[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                              # also uploads the tables
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for batch, want in zip(batches + batches[:1], wants + wants[:1]):
        raw.copy_(batch)
        for x in (stream, nbytes, workspace):              # poison
            x.view(torch.uint8).fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        _assert_streams((stream, nbytes), want, "replay")
        assert all(bool((stream[b, int(nbytes[b]):] == 0x5A).all()) for b in range(3))


def test_refusals(native):
    from aiko_services_amd.ops import jpeg as J
    fmt, H, W = "i420", 17, 23
    raw = S.frames(fmt, H, W).cuda()
    cap, seg_cap = J.capacities(fmt, H, W)

    def refuse(match, raw=raw, error=RuntimeError, H=H, W=W, fmt=fmt, quality=90, **kw):
        with pytest.raises(error, match=match):
            J.jpeg_encode(raw, H, W, fmt, quality, **kw)

    refuse("raw uint8", raw=raw.to(torch.int8))
    refuse("raw uint8", raw=torch.zeros(3, 2 * raw.shape[1], dtype=torch.uint8, device="cuda")[:, ::2])
    refuse("stream uint8", stream=torch.empty(3, cap, dtype=torch.int8, device="cuda"))
    refuse("stream uint8", stream=torch.empty(3, 2 * cap, dtype=torch.uint8, device="cuda")[:, ::2], cap=cap)
    refuse("nbytes int32", nbytes=torch.empty(3, dtype=torch.int64, device="cuda"))
    refuse("nbytes int32", nbytes=torch.empty(4, dtype=torch.int32, device="cuda"))
    refuse("workspace uint8", workspace=torch.empty(J.workspace_bytes(fmt, H, W, 3) - 1, dtype=torch.uint8, device="cuda"))
    refuse("workspace uint8", workspace=torch.empty(J.workspace_bytes(fmt, H, W, 3) // 4 + 1, dtype=torch.int32,
                                                    device="cuda"))
    refuse("workspace uint8", workspace=torch.empty(J.workspace_bytes(fmt, H, W, 3) + 4, dtype=torch.uint8,
                                                    device="cuda")[1:])            # not 4-byte aligned
    refuse("GPU tensor", raw=raw.cpu(), stream=torch.empty(3, cap, dtype=torch.uint8, device="cuda"))
    refuse("GPU tensor", stream=torch.empty(3, cap, dtype=torch.uint8))
    refuse("GPU tensor", nbytes=torch.empty(3, dtype=torch.int32))
    if torch.cuda.device_count() > 1:
        refuse("device", stream=torch.empty(3, cap, dtype=torch.uint8, device="cuda:1"))
    # no output over an input or another output
    shared = torch.zeros(3 * cap + raw.numel(), dtype=torch.uint8, device="cuda")
    refuse("stream and raw overlap", raw=shared[:raw.numel()].view(3, -1), stream=shared[8:8 + 3 * cap].view(3, cap))
    refuse("workspace and stream overlap", stream=shared[:3 * cap].view(3, cap), workspace=shared)
    need = J.workspace_bytes(fmt, H, W, 3)
    whole = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    refuse("workspace and nbytes overlap", nbytes=whole[need - 4:need + 8].view(torch.int32), workspace=whole[:need])
    # values: Python errors
    for bad in ("nv12", "yuyv", "rgb"):
        refuse("format", error=ValueError, fmt=bad)
    for bad in (0, 101, True, 90.0):
        refuse("quality", error=ValueError, quality=bad)
    refuse("raw", error=ValueError, H=H + 1)
    refuse("raw", error=ValueError, raw=raw[0])
    refuse("stream", error=ValueError, stream=torch.empty(4, cap, dtype=torch.uint8, device="cuda"))
    refuse("stream", error=ValueError, stream=torch.empty(3, cap, dtype=torch.uint8, device="cuda"), cap=cap + 1)
    refuse("seg_cap", error=ValueError, seg_cap=0)
    refuse("seg_cap", error=ValueError, seg_cap=J.MAX_SEG_CAP + 1)
    refuse("cap", error=ValueError, cap=0)
    refuse("height", error=ValueError, raw=torch.zeros(1, 3 * 4097, dtype=torch.uint8, device="cuda"), H=1, W=4097,
           fmt="i444")
    # the operator's own bounds, past the Python layer
    tables, head = J.device_tables(fmt, H, W, 90, "cuda")
    outs = (torch.empty(3, cap, dtype=torch.uint8, device="cuda"), torch.empty(3, dtype=torch.int32, device="cuda"),
            torch.empty(J.workspace_bytes(fmt, H, W, 3, J.MAX_SEG_CAP + 1), dtype=torch.uint8, device="cuda"))
    for args, text in (((raw, H, W, 0, tables, head, seg_cap), "fmt 1"),
                       ((raw, H, W, 3, tables, head, seg_cap), "fmt 1"),
                       ((raw, H, W, 1, tables, head, J.MAX_SEG_CAP + 1), "seg_cap"),
                       ((raw, H, W, 1, tables, head, 0), "seg_cap"),
                       ((raw, H, W, 1, tables, head - 1, seg_cap), "tables uint8"),
                       ((raw, H, W, 1, tables[:-1], head, seg_cap), "tables uint8"),
                       ((raw, H, W, 1, tables.to(torch.int8), head, seg_cap), "tables uint8"),
                       ((torch.zeros(1, 3 * 4097, dtype=torch.uint8, device="cuda"), 1, 4097, 2, tables, head, seg_cap),
                        "width <= 4096"),
                       ((raw, 0, W, 1, tables, head, seg_cap), "1 <= height")):
        with pytest.raises(RuntimeError, match=text):
            torch.ops.aiko.jpeg_encode_out(*args, *outs)
    # inside them: the extremes of quality, the smallest capacities (everything overflows, nothing faults)
    for quality in (1, 100):
        J.jpeg_encode(raw, H, W, fmt, quality)
    got = J.jpeg_encode(raw, H, W, fmt, 90, cap=1, seg_cap=1)
    torch.cuda.synchronize()
    assert got[1].tolist() == [-1, -1, -1]


# ---- the elements ---------------------------------------------------------------------------------

VISION = "aiko_services_amd.elements.gpu.vision"
JPEG = "aiko_services_amd.elements.gpu.jpeg"
EXAMPLE = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/yolo/yolo_mjpeg_gpu.json"


def _create(definition):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<jpeg>", parse_pipeline_definition_dict(definition), None, None, "j", [], 0,
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


@pytest.mark.parametrize("subsampling,lanes", [("420", 1), ("444", 2)])
def test_jpeg_encode_element_equals_direct_calls(native, subsampling, lanes):
    from aiko_services_amd.ops import jpeg as J
    from aiko_services_amd.ops.yuv import rgb_to_yuv
    b, h, w, frames, quality = 2, 18, 40, 5, 80
    fmt = "i" + subsampling
    d = {"version": 0, "name": "p_jpeg", "runtime": "python", "graph": ["(SyntheticFrames JpegEncode)"],
         "parameters": {"gpu_lanes": lanes},
         "elements": [
             _element("SyntheticFrames", VISION, [], [("images", "tensor"), ("t_submit", "float")],
                      {"batch": b, "height": h, "width": w, "pool": 2, "seed": 4}),
             _element("JpegEncode", JPEG, ["images"], [("images", "tensor"), ("nbytes", "tensor")],
                      {"quality": quality, "subsampling": subsampling})]}
    p, q = _create(d)
    p.response_swag = True
    seen = _spy(p.pipeline_graph.get_node("JpegEncode").element)
    cap = J.capacities(fmt, h, w)[0]
    for i in range(frames):
        p.process_frame({"stream_id": "j", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        torch.cuda.synchronize()
        assert tuple(swag["images"].shape) == (b, cap) and tuple(swag["nbytes"].shape) == (b,)
        direct = J.jpeg_encode(rgb_to_yuv(seen[i], fmt, "jpeg"), h, w, fmt, quality)
        torch.cuda.synchronize()
        assert int(direct[1].min()) > 0
        _assert_streams((swag["images"], swag["nbytes"]), (direct[0].cpu(), direct[1].cpu()), f"frame {i}")
        if i == 0:                                          # and the whole chain against the references
            _assert_streams(direct, _ref(S.raw_from_rgb(seen[0].cpu(), fmt), h, w, fmt, quality), "reference")
    assert p.share["gpu_lanes"] == lanes


def test_jpeg_encode_element_raw_input_and_diagnostics(native):
    from aiko_services_amd.pipeline.stream import StreamEvent
    h, w = 17, 23
    d = {"version": 0, "name": "p_jpeg", "runtime": "python", "graph": ["(JpegEncode JpegResults)"], "parameters": {},
         "elements": [
             _element("JpegEncode", JPEG, ["images"], [("images", "tensor"), ("nbytes", "tensor")],
                      {"quality": 50, "input": "i444", "height": h, "width": w, "cap": S.roomy("i444", h, w)["cap"]}),
             _element("JpegResults", JPEG, ["images", "nbytes"],
                      [("images", "[image]"), ("nbytes", "[int]"), ("format", "str")], {})]}
    p, _ = _create(d)
    encode = p.pipeline_graph.get_node("JpegEncode").element
    results = p.pipeline_graph.get_node("JpegResults").element
    raw = S.frames("i444", h, w)
    want = _ref(raw, h, w, "i444", 50, cap=S.roomy("i444", h, w)["cap"])
    assert int(want[1].min()) > 0
    event, out = encode.process_frame(None, raw.cuda())
    assert event == StreamEvent.OKAY
    torch.cuda.synchronize()
    _assert_streams((out["images"], out["nbytes"]), want, "raw input")
    event, host = results.process_frame(None, out["images"], out["nbytes"])
    assert event == StreamEvent.OKAY and host["format"] == "jpeg" and host["nbytes"] == want[1].tolist()
    for b, frame in enumerate(host["images"]):
        assert bytes(frame) == S.stream_bytes(*want, b) and S.decode(bytes(frame)).shape == (h, w, 3)
    assert results.bytes_downloaded == 3 * int(want[1].max())
    # an overflowed frame is an error that names it and the capacity
    small = torch.full_like(out["nbytes"], 700)
    small[1] = -1
    event, host = results.process_frame(None, out["images"], small)
    assert event == StreamEvent.ERROR and "frame 1" in host["diagnostic"] and str(out["images"].shape[1]) in host["diagnostic"]
    for bad, text in ((raw.cuda().float(), "images uint8"), (raw.cuda()[:, :-1].contiguous(), "raw i444"),
                      (raw, "images uint8"), (None, "images uint8")):
        event, out = encode.process_frame(None, bad)
        assert event == StreamEvent.ERROR and text in out["diagnostic"], out
    for parameters, text in (({"quality": 0}, "quality"), ({"subsampling": "422"}, "subsampling"),
                             ({"input": "nv12"}, "input"), ({"input": "i420"}, "height and width"),
                             ({"input": "i420", "subsampling": "444", "height": 8, "width": 8}, "does not apply")):
        d["elements"][0]["parameters"] = parameters
        with pytest.raises(Exception, match=text):
            _create(d)


def test_example_pipeline_writes_an_mjpeg_avi(native, tmp_path):
    """The frames of the .avi are the reference's streams of the frames that were encoded, and decode to
    within the fidelity bound of test_jpeg_reference.py: Pillow's own encoder less 0.5 dB."""
    from aiko_services_amd.elements.media.avi import _parse, avi_info, read_avi
    b, h, w, frames = 2, 240, 320, 3
    path = tmp_path / "out.avi"
    d = json.loads(EXAMPLE.read_text())
    assert d["graph"] == ["(SyntheticFrames YoloDetector DetectionOverlay JpegEncode JpegResults VideoWriteFile)"]
    by_name = {e["name"]: e for e in d["elements"]}
    assert by_name["VideoWriteFile"]["parameters"]["format"] == "jpeg" and by_name["VideoWriteFile"]["parameters"]["raw"]
    quality = by_name["JpegEncode"]["parameters"]["quality"]
    by_name["SyntheticFrames"]["parameters"].update(batch=b, height=h, width=w)
    by_name["YoloDetector"]["parameters"].update(autotune=False)
    by_name["VideoWriteFile"]["parameters"].update(data_targets=f"file://{path}", rate=25)
    p, q = _create(d)
    seen = _spy(p.pipeline_graph.get_node("JpegEncode").element)
    for i in range(frames):
        p.process_frame({"stream_id": "j", "frame_id": i}, {})
        info, out = q.get_nowait()
        assert info["state"] == 0, out
    writer = p.pipeline_graph.get_node("VideoWriteFile").element
    writer.stop_stream(p.stream_leases["j"].stream, "j")
    info = avi_info(path)
    assert (info["width"], info["height"], info["frames"], info["compression"]) == (w, h, frames * b, b"MJPG")
    back = read_avi(path)
    sources = torch.cat(seen).cpu()
    assert back.shape == (frames * b, h, w, 3) == tuple(sources.shape)
    for i in range(frames * b):
        ours = S.psnr(back[i], sources[i].numpy())
        theirs = S.psnr(S.decode(S.pillow_encode(sources[i], "i420", quality)), sources[i].numpy())
        print(f"avi frame {i}: {ours:.2f} dB, Pillow {theirs:.2f} dB")
        assert ours >= theirs - 0.5
    # the first chunk of the file is the reference's stream of the first frame, byte for byte
    want = _ref(S.raw_from_rgb(sources[0], "i420"), h, w, "i420", quality)
    _, chunks = _parse(path)
    data = path.read_bytes()
    assert data[chunks[0][0]:chunks[0][0] + chunks[0][1]] == S.stream_bytes(*want)
    assert path.stat().st_size < frames * b * h * w * 3 // 2
