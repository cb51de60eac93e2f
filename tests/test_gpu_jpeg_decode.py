"""jpeg_decode on the device against ``ops.reference.jpeg_decode_ref``, bit for bit: planes and status."""
import queue
from pathlib import Path

import pytest
import torch

import jpeg_decode_scenes as DS
import jpeg_scenes as S
from kernel_guard import guarded

pytestmark = pytest.mark.gpu


def _cuda(*tensors):
    return tuple(t.cuda() for t in tensors)


def _assert_frames(got, want, where):
    raw, status = got[0].cpu(), got[1].cpu()
    assert status.tolist() == want[1].tolist(), f"{where}: status {status.tolist()}, reference {want[1].tolist()}"
    for b in range(raw.shape[0]):
        if int(want[1][b]):
            continue                                        # unspecified within its own row
        if not torch.equal(raw[b], want[0][b]):
            first = int(torch.nonzero(raw[b] != want[0][b])[0])
            raise AssertionError(f"{where}: frame {b} differs from byte {first}: {int(raw[b, first])}, reference "
                                 f"{int(want[0][b, first])} ({int((raw[b] != want[0][b]).sum())} bytes differ)")


@pytest.mark.parametrize("fmt", DS.FORMATS)
@pytest.mark.parametrize("H,W", DS.SHAPES)
def test_frames_equal_reference(native, fmt, H, W):
    """Every kind of stream on its own, with the launches sized by its own restart interval, then all of
    them in one batch (tables and DRI differing per frame) sized for any stream."""
    from aiko_services_amd.ops import jpeg_decode as D
    from aiko_services_amd.ops.reference import jpeg_decode_ref
    W = DS.width(fmt, W)
    frames = []
    for kind in DS.KINDS:
        if not DS.streams(fmt, H, W, kind):
            continue
        data, nbytes, desc, plan = DS.packed(fmt, H, W, kind)
        want = DS.reference(fmt, H, W, kind)
        assert not want[1].any()
        frames += DS.streams(fmt, H, W, kind)
        if kind == "pillow_rst1":                           # the most intervals a frame can have
            assert plan.restart_interval == 1
            got = D.jpeg_decode(*_cuda(data, nbytes, desc), H, W, fmt)
        else:
            got = D.jpeg_decode(*_cuda(data, nbytes, desc), H, W, fmt, restart_interval=plan.restart_interval)
        torch.cuda.synchronize()
        _assert_frames(got, want, kind)
    data, nbytes, desc, _ = D.pack(frames)
    _assert_frames(D.jpeg_decode(*_cuda(data, nbytes, desc), H, W, fmt), jpeg_decode_ref(data, nbytes, desc, H, W, fmt),
                   "all kinds in one batch")


def test_tables_per_frame_and_one_descriptor_for_all(native):
    from aiko_services_amd.ops import jpeg as J
    from aiko_services_amd.ops import jpeg_decode as D
    from aiko_services_amd.ops.reference import jpeg_decode_ref
    fmt, H, W = "i420", 40, 56
    rgb = [S.smooth_noise_rgb(H, W, s) for s in range(4)]
    frames = [DS.pillow_stream(rgb[0], fmt, 30), DS.pillow_stream(rgb[1], fmt, 90),
              DS.pillow_stream(rgb[2], fmt, 90, optimize=True), DS.pillow_stream(rgb[3], fmt, 30, optimize=True)]
    data, nbytes, desc, _ = D.pack(frames)
    assert len({bytes(d.tolist()) for d in desc}) == 4
    want = jpeg_decode_ref(data, nbytes, desc, H, W, fmt)
    assert not want[1].any()
    _assert_frames(D.jpeg_decode(*_cuda(data, nbytes, desc), H, W, fmt), want, "tables per frame")
    # the device-to-device case: the encoder's streams, one descriptor from the header it writes
    raw = torch.cat([S.raw_from_rgb(x, fmt) for x in rgb])
    stream, lengths = J.jpeg_encode(raw.cuda(), H, W, fmt, 75)
    plan = D.parse(J.header(fmt, H, W, 75))
    one = D.plan_bytes(plan)[None]
    got = D.jpeg_decode(stream, lengths, one.cuda(), H, W, fmt, restart_interval=plan.restart_interval)
    torch.cuda.synchronize()
    want = jpeg_decode_ref(stream.cpu(), lengths.cpu(), one, H, W, fmt)
    assert not want[1].any()
    _assert_frames(got, want, "one descriptor")
    assert int((got[0].cpu().int() - raw.int()).abs().max()) < 64          # it is the picture that went in


def _corrupt_batch():
    from aiko_services_amd.ops import jpeg_decode as D
    hand = DS.corrupt_handful()
    good, n = hand["valid"]
    order = ["valid", "truncated", "cut_short_with_eoi", "removed_rst", "valid", "swapped_rst", "stray_marker",
             "invalid_code", "run_leaves_block", "zero_length", "overflowed_encode", "valid"]
    plan = D.parse(good)
    return DS.pack_raw([hand[k][0] for k in order], [hand[k][1] for k in order], plan), plan


def test_corrupt_frames_in_a_batch_and_guard_bands(native):
    """The corrupt streams (each went through the sanitizers on the CPU, test_jpeg_decode_core_native.py) in
    the middle of a batch: their status is the reference's, the neighbours are exact, nothing outside a
    tensor changes, and the poison behind ``nbytes`` reaches no output."""
    from aiko_services_amd.ops import jpeg_decode as D
    from aiko_services_amd.ops.reference import jpeg_decode_ref
    from aiko_services_amd.ops.yuv import frame_bytes
    fmt, H, W = DS.CORRUPT_SHAPE
    (data, nbytes, desc), plan = _corrupt_batch()
    B = data.shape[0]
    want = jpeg_decode_ref(data, nbytes, desc, H, W, fmt)
    assert want[1].tolist() == [0, 1, 4, 1, 0, 1, 16, 2, 8, 1, 1, 0]
    poisoned = data.clone()
    for b in range(B):
        poisoned[b, max(int(nbytes[b]), 0):] = 0xA5
    checks = []

    def g(shape, dtype, values=None, name=""):
        view, check = guarded(shape, dtype, "cuda", values=values, name=name)
        checks.append(check)
        return view

    for ri in (plan.restart_interval, None):
        checks.clear()
        gdata, gn, gdesc = g(data.shape, torch.uint8, poisoned, "data"), g((B,), torch.int32, nbytes, "nbytes"), \
            g(desc.shape, torch.uint8, desc, "desc")
        raw, status = g((B, frame_bytes(fmt, H, W)), torch.uint8, name="raw"), g((B,), torch.int32, name="status")
        workspace = g((D.workspace_bytes(fmt, H, W, B, ri),), torch.uint8, name="workspace")
        D.jpeg_decode(gdata, gn, gdesc, H, W, fmt, restart_interval=ri, raw=raw, status=status, workspace=workspace)
        torch.cuda.synchronize()
        for check in checks:
            check()
        _assert_frames((raw, status), want, f"guarded, restart_interval {ri}")
        assert torch.equal(gdata.cpu(), poisoned) and torch.equal(gdesc.cpu(), desc) and torch.equal(gn.cpu(), nbytes)
    # a stream with more intervals than the call provides for: bit 1
    got = D.jpeg_decode(*_cuda(data[:1], nbytes[:1], desc[:1]), H, W, fmt, restart_interval=0)
    assert got[1].tolist() == [1]


def test_capture_and_replay(native):
    from aiko_services_amd.ops import jpeg_decode as D
    from aiko_services_amd.ops.reference import jpeg_decode_ref
    from aiko_services_amd.ops.yuv import frame_bytes
    fmt, H, W = "i420", 40, 56
    batches = []
    for seed, kw in ((0, {"restart_marker_rows": 1}), (1, {"optimize": True}), (2, {})):
        frames = [DS.pillow_stream(S.smooth_noise_rgb(H, W, 3 * seed + k), fmt, 60 + 10 * k, **kw) for k in range(3)]
        batches.append(D.pack(frames, out=(torch.zeros(3, 8192, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32),
                                           torch.zeros(3, D.PLAN_BYTES, dtype=torch.uint8)))[:3])
    wants = [jpeg_decode_ref(*b, H, W, fmt) for b in batches]
    data, nbytes, desc = (torch.empty_like(t, device="cuda") for t in batches[0])
    raw = torch.empty(3, frame_bytes(fmt, H, W), dtype=torch.uint8, device="cuda")
    status = torch.empty(3, dtype=torch.int32, device="cuda")
    workspace = torch.empty(D.workspace_bytes(fmt, H, W, 3), dtype=torch.uint8, device="cuda")

    def run():
        D.jpeg_decode(data, nbytes, desc, H, W, fmt, raw=raw, status=status, workspace=workspace)

    for dst, src in zip((data, nbytes, desc), batches[0]):
        dst.copy_(src)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    eager = (raw.clone(), status.clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for batch, want in zip(batches + batches[:1], wants + wants[:1]):
        for dst, src in zip((data, nbytes, desc), batch):
            dst.copy_(src)
        for x in (raw, status, workspace):                 # poison
            x.view(torch.uint8).fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        _assert_frames((raw, status), want, "replay")
    assert torch.equal(raw, eager[0]) and torch.equal(status, eager[1])


def test_refusals(native):
    from aiko_services_amd.ops import jpeg_decode as D
    fmt, H, W = "i420", 17, 23
    data, nbytes, desc, plan = DS.packed(fmt, H, W, "pillow")
    data, nbytes, desc = _cuda(data, nbytes, desc)
    B, cap = data.shape
    need = D.workspace_bytes(fmt, H, W, B)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")  # noqa: E731

    def refuse(match, error=RuntimeError, data=data, nbytes=nbytes, desc=desc, H=H, W=W, fmt=fmt, **kw):
        with pytest.raises(error, match=match):
            D.jpeg_decode(data, nbytes, desc, H, W, fmt, **kw)

    refuse("data uint8", data=data.to(torch.int8))
    refuse("data uint8", data=u8(B, 2 * cap)[:, ::2])
    refuse("nbytes int32", nbytes=nbytes.long())
    refuse("desc uint8", desc=desc.to(torch.int8))
    refuse("desc uint8", desc=u8(B, 2 * D.PLAN_BYTES)[:, ::2])
    refuse("desc uint8", desc=u8(B * D.PLAN_BYTES + 4)[1:1 + B * D.PLAN_BYTES].view(B, -1))       # not 4-byte aligned
    refuse("raw uint8", raw=torch.empty(B, D.frame_bytes(fmt, H, W), dtype=torch.int8, device="cuda"))
    refuse("status int32", status=torch.empty(B, dtype=torch.int64, device="cuda"))
    refuse("status int32", status=torch.empty(B + 1, dtype=torch.int32, device="cuda"))
    refuse("workspace uint8", workspace=u8(need - 1))
    refuse("workspace uint8", workspace=u8(need + 16)[4:])                                          # not 16-byte aligned
    refuse("workspace uint8", workspace=torch.empty(need // 4 + 4, dtype=torch.int32, device="cuda"))
    refuse("GPU tensor", data=data.cpu())
    refuse("GPU tensor", status=torch.empty(B, dtype=torch.int32))
    shared = u8(B * cap + need + 64)
    refuse("workspace and data overlap", data=shared[:B * cap].view(B, cap), workspace=shared[B * cap - 16:][:need + 16])
    refuse("raw and desc overlap", desc=shared[:B * D.PLAN_BYTES].view(B, -1),
           raw=shared[16:16 + B * D.frame_bytes(fmt, H, W)].view(B, -1))
    whole = u8(need + 16)
    refuse("workspace and status overlap", status=whole[need - 16:need - 16 + 4 * B].view(torch.int32), workspace=whole[:need])
    # values: Python errors
    for bad in ("nv12", "rgb"):
        refuse("format", error=ValueError, fmt=bad)
    refuse("even width", error=ValueError, fmt="yuyv")
    refuse("width", error=ValueError, W=4097)
    refuse("restart_interval", error=ValueError, restart_interval=-1)
    refuse("desc", error=ValueError, desc=desc[:, :-1])
    refuse("desc", error=ValueError, desc=desc[:1].repeat(B + 1, 1))
    refuse("nbytes", error=ValueError, nbytes=nbytes[:-1])
    refuse("raw", error=ValueError, raw=u8(B, D.frame_bytes(fmt, H, W) + 1))
    # the operator's own bounds, past the Python layer
    outs = (u8(B, D.frame_bytes(fmt, H, W)), torch.empty(B, dtype=torch.int32, device="cuda"), u8(need))
    mcus = 2 * 2
    for args, text in (((H, W, 0, mcus), "fmt 1"), ((H, W, 4, mcus), "fmt 1"), ((H, W, 1, 0), "max_intervals"),
                       ((H, W, 1, mcus + 1), "max_intervals"), ((0, W, 1, 1), "1 <= height"),
                       ((H, 4097, 1, 1), "width <= 4096"), ((H, W, 3, 1), "even width")):
        with pytest.raises(RuntimeError, match=text):
            torch.ops.aiko.jpeg_decode_out(data, nbytes, desc, *args, *outs)


# ---- the element ----------------------------------------------------------------------------------

JPEG = "aiko_services_amd.elements.gpu.jpeg"
JPEG_IN = "aiko_services_amd.elements.gpu.jpeg_in"
VISION = "aiko_services_amd.elements.gpu.vision"
VIDEO = "aiko_services_amd.elements.media.video_io"
EXAMPLE = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/yolo/yolo_mjpeg_in_gpu.json"


def _create(definition):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<jpeg_in>", parse_pipeline_definition_dict(definition), None, None, "j", [], 0,
                                     None, 60, queue_response=q)
    return p, q


def _element(name, module, inputs, outputs, parameters):
    return {"name": name, "input": [{"name": n, "type": "tensor"} for n in inputs],
            "output": [{"name": n, "type": t} for n, t in outputs], "parameters": parameters,
            "deploy": {"local": {"module": module}}}


def test_avi_through_video_read_file_and_jpeg_decode(native, tmp_path):
    import json

    from aiko_services_amd.elements.media.avi import AviWriter
    from aiko_services_amd.elements.media.video_io import iter_video_frames
    from aiko_services_amd.ops import jpeg_decode as D
    from aiko_services_amd.ops.reference import jpeg_decode_ref, yuv_to_rgb_ref
    from aiko_services_amd.pipeline.stream import StreamEvent
    example = json.loads(EXAMPLE.read_text())
    assert example["graph"] == ["(VideoReadFile JpegDecode YoloDetector DetectionOverlay JpegEncode JpegResults "
                                "VideoWriteFile)"]
    by_name = {e["name"]: e for e in example["elements"]}
    assert by_name["VideoReadFile"]["parameters"]["raw"] is True
    assert by_name["JpegDecode"]["deploy"]["local"]["module"] == JPEG_IN
    fmt, H, W = "i420", 34, 50
    coded = [DS.pillow_stream(S.structured_rgb(H, W, s), fmt, 85, **kw)
             for s, kw in enumerate(({}, {"optimize": True}, {"restart_marker_rows": 1}, {}))]
    path = tmp_path / "in.avi"
    with AviWriter(path, W, H, 25.0) as writer:
        for f in coded:
            writer.write_jpeg(f)
    chunks = list(iter_video_frames(path, raw=True))
    assert [c.tobytes() for c in chunks] == coded
    d = {"version": 0, "name": "p_jpeg_in", "runtime": "python", "graph": ["(JpegDecode)"], "parameters": {},
         "elements": [_element("JpegDecode", JPEG_IN, ["images"], [("images", "tensor"), ("status", "tensor")],
                               by_name["JpegDecode"]["parameters"])]}
    p, _ = _create(d)
    element = p.pipeline_graph.get_node("JpegDecode").element
    for batch in (chunks[:2], chunks[2:], chunks[1:3], chunks[:2]):
        event, out = element.process_frame(None, batch)
        assert event == StreamEvent.OKAY, out
        torch.cuda.synchronize()
        data, nbytes, desc, _ = D.pack(batch)
        raw, status = jpeg_decode_ref(data, nbytes, desc, H, W, fmt)
        assert out["status"].tolist() == [0, 0] == status.tolist()
        assert tuple(out["images"].shape) == (2, H, W, 3)
        assert torch.equal(out["images"].cpu(), yuv_to_rgb_ref(raw, H, W, fmt, "jpeg"))
    assert element.bytes_uploaded == sum(len(c) for c in chunks[:2] + chunks[2:] + chunks[1:3] + chunks[:2])
    # streams the decoder does not take, and a change of shape, are errors that say why
    from PIL import Image
    import io
    buf = io.BytesIO()
    Image.fromarray(S.structured_rgb(H, W).numpy()).save(buf, format="JPEG", progressive=True)
    for bad, text in (([coded[0], buf.getvalue()], "progressive"), ([DS.pillow_stream(S.structured_rgb(H, W + 2), fmt, 85)], "34 x 52"),
                      ([DS.pillow_stream(S.structured_rgb(H, W), "i444", 85)], "i444"), (torch.zeros(4), "list of coded frames")):
        event, out = element.process_frame(None, bad)
        assert event == StreamEvent.ERROR and text in out["diagnostic"], out
    # output: raw
    d["elements"][0]["parameters"] = {"output": "raw", "subsampling": "420", "height": H, "width": W}
    element = _create(d)[0].pipeline_graph.get_node("JpegDecode").element
    event, out = element.process_frame(None, chunks[:2])
    torch.cuda.synchronize()
    data, nbytes, desc, _ = D.pack(chunks[:2])
    assert event == StreamEvent.OKAY and torch.equal(out["images"].cpu(), jpeg_decode_ref(data, nbytes, desc, H, W, fmt)[0])
    for parameters, text in (({"input": "file"}, "input"), ({"output": "bgr"}, "output"), ({"subsampling": "411"}, "subsampling"),
                             ({"input": "device"}, "height and width"),
                             ({"input": "device", "subsampling": "422", "height": 8, "width": 8}, "JpegEncode writes")):
        d["elements"][0]["parameters"] = parameters
        with pytest.raises(Exception, match=text):
            _create(d)


@pytest.mark.parametrize("subsampling", ["420", "444"])
def test_jpeg_encode_then_jpeg_decode_on_the_device(native, subsampling):
    from aiko_services_amd.ops import jpeg as J
    from aiko_services_amd.ops import jpeg_decode as D
    from aiko_services_amd.ops.reference import jpeg_decode_ref, jpeg_encode_ref, yuv_to_rgb_ref
    b, h, w, quality = 2, 18, 40, 80
    fmt = "i" + subsampling
    d = {"version": 0, "name": "p_jpeg_loop", "runtime": "python", "graph": ["(SyntheticFrames JpegEncode JpegDecode)"],
         "parameters": {},
         "elements": [
             _element("SyntheticFrames", VISION, [], [("images", "tensor"), ("t_submit", "float")],
                      {"batch": b, "height": h, "width": w, "pool": 2, "seed": 4}),
             _element("JpegEncode", JPEG, ["images"], [("images", "tensor"), ("nbytes", "tensor")],
                      {"quality": quality, "subsampling": subsampling}),
             _element("JpegDecode", JPEG_IN, ["images", "nbytes"], [("images", "tensor"), ("status", "tensor")],
                      {"input": "device", "quality": quality, "subsampling": subsampling, "height": h, "width": w})]}
    p, q = _create(d)
    p.response_swag = True
    encode = p.pipeline_graph.get_node("JpegEncode").element
    inner, seen = encode.process_frame, []

    def spy(stream, images, *args, **kw):
        seen.append(images.clone())
        return inner(stream, images, *args, **kw)

    encode.process_frame = spy
    one = D.plan_bytes(D.parse(J.header(fmt, h, w, quality)))[None]
    for i in range(3):
        p.process_frame({"stream_id": "j", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        torch.cuda.synchronize()
        stream, nbytes = jpeg_encode_ref(S.raw_from_rgb(seen[i].cpu(), fmt), h, w, fmt, quality)
        raw, status = jpeg_decode_ref(stream, nbytes, one, h, w, fmt)
        assert swag["status"].tolist() == [0, 0] == status.tolist()
        assert torch.equal(swag["images"].cpu(), yuv_to_rgb_ref(raw, h, w, fmt, "jpeg")), f"frame {i}"
