"""The antialiased resize on the MI355X (``scale_ops.hip``): bit for bit against
``scale_frames_ref`` on the shared scenes (scale_scenes.py) with all five filters, whole frame and
box, through a view one byte off alignment, over several tiles with partial last ones, at
``MAX_TAPS``, under hipGraph replay with the frames rewritten on the device, between guard bands,
the refusals, ``ImageResize`` with ``filter`` against its host branch, and the FrameScale element
in its example pipeline against the same kernel called directly.  No test compares the kernel with
itself; Pillow is not needed here."""
import json
import queue
from pathlib import Path

import numpy as np
import pytest
import torch

import scale_scenes as S
from kernel_guard import guarded

pytestmark = pytest.mark.gpu


def diff_report(name, got, ref):
    diff = (got != ref)
    print(f"scale {name}: {int(diff.sum())} of {diff.numel()} bytes differ {torch.nonzero(diff)[:4].tolist()}")


@pytest.mark.parametrize("f", S.FILTER_NAMES)
@pytest.mark.parametrize("pair", S.PAIRS, ids=lambda p: "{}x{}-{}x{}".format(*p))
def test_equals_reference(native, pair, f):
    """Whole frame and box, on fresh tensors and on a batch that starts one byte into a larger
    buffer (no row of it is aligned to anything)."""
    from aiko_services_amd.ops.scale import scale_frames
    h, w, ho, wo = pair
    host = S.frames(h, w)
    before = host.clone()
    frames = host.cuda()
    buffer = torch.zeros(host.numel() + 64, dtype=torch.uint8, device="cuda")
    view = buffer[1:1 + host.numel()].view(host.shape)
    view.copy_(frames)
    assert view.is_contiguous() and view.data_ptr() % 2 == 1
    for boxed in (False, True):
        case = (pair, f, boxed)
        ref = S.reference(case)
        got = scale_frames(frames, (ho, wo), f, S.box(case))
        offset = scale_frames(view, (ho, wo), f, S.box(case))
        torch.cuda.synchronize()
        diff_report(S.case_id(case), got.cpu(), ref)
        assert torch.equal(got.cpu(), ref), S.case_id(case)
        assert torch.equal(offset.cpu(), ref), S.case_id(case) + " (view one byte in)"
    assert torch.equal(frames.cpu(), before) and torch.equal(S.frames(h, w), before)
    assert not buffer[0].item() and not buffer[1 + host.numel():].any().item()


def test_several_tiles_with_partial_last_ones(native):
    """97 x 131 -> 70 x 150 is two tiles of rows (64 + 6) and three of columns (64 + 64 + 22); with
    ``lanczos`` 480 x 640 -> 224 x 224 is four by four.  The plan says so, and the kernel's output
    over those tiles is the reference's."""
    from aiko_services_amd.ops.scale import scale_frames, scale_plan
    for pair, f, tiles in (((97, 131, 70, 150), "bicubic", (2, 3)), ((480, 640, 224, 224), "lanczos", (4, 4))):
        h, w, ho, wo = pair
        plan = scale_plan(h, w, (ho, wo), f, device="cuda")
        assert (-(-ho // plan.tile_rows), -(-wo // plan.tile_cols)) == tiles, plan[5:]
        assert ho % plan.tile_rows and wo % plan.tile_cols                     # a partial last tile each way
        got = scale_frames(S.frames(h, w).cuda(), (ho, wo), f)
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), S.reference((pair, f, False)))


def test_max_taps_and_one_above(native):
    """4096 rows -> 1 with ``box`` is MAX_TAPS = 4097 taps: one output row per tile, twelve columns
    wide, 147456 bytes of LDS.  ``lanczos`` at 97:1 (583 taps) narrows the tile until its window fits the
    32 KiB a tile should take.  One tap above MAX_TAPS is refused."""
    from aiko_services_amd.ops import scale as Sc
    from aiko_services_amd.ops.reference import scale_frames_ref
    g = torch.Generator().manual_seed(11)
    frames = torch.randint(0, 256, (S.B, 4096, 20, 3), dtype=torch.uint8, generator=g)
    plan = Sc.scale_plan(4096, 20, (1, 7), "box", device="cuda")
    assert plan.vk.shape == (1, Sc.MAX_TAPS) and (plan.tile_rows, plan.tile_cols, plan.win_rows) == (1, 12, 4096)
    got = Sc.scale_frames(frames.cuda(), (1, 7), "box")
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), scale_frames_ref(frames, (1, 7), "box"))
    tall = frames[:, :1552]
    plan = Sc.scale_plan(1552, 20, (16, 7), "lanczos", device="cuda")
    assert plan.vk.shape == (16, 583) and plan.tile_cols < 64 and plan.win_rows >= 583
    assert plan.win_rows * plan.tile_cols * 3 <= Sc.TILE_LDS
    got = Sc.scale_frames(tall.contiguous().cuda(), (16, 7), "lanczos")
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), scale_frames_ref(tall, (16, 7), "lanczos"))
    with pytest.raises(ValueError, match="MAX_TAPS"):
        Sc.scale_frames(torch.zeros(1, 4098, 20, 3, dtype=torch.uint8, device="cuda"), (1, 7), "box")
    with pytest.raises(ValueError, match="MAX_TAPS"):
        Sc.scale_frames(torch.zeros(1, 20, 4098, 3, dtype=torch.uint8, device="cuda"), (7, 1), "box")


def test_frames_rewritten_under_graph_replay(native):
    from aiko_services_amd.ops.scale import scale_frames
    pair, f = (97, 131, 70, 150), "lanczos"
    h, w, ho, wo = pair
    case = (pair, f, True)
    frames = S.frames(h, w).cuda().clone()
    out = torch.empty(S.B, ho, wo, 3, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scale_frames(frames, (ho, wo), f, S.box(case), out=out)    # the plan is made and uploaded here
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scale_frames(frames, (ho, wo), f, S.box(case), out=out)
    previous = None
    for seed in (0, 1, 2):
        frames.copy_(S.frames(h, w, seed).cuda())
        out.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), S.reference(case, seed)), seed
        if previous is not None:
            assert (out != previous).any()
        previous = out.clone()


@pytest.mark.parametrize("width", [53, 64])
@pytest.mark.parametrize("size", [(91, 17), (37, 17), (91, None)], ids=["both", "horizontal", "vertical"])
def test_guard_bands(native, width, size):
    """Frames, the four tables and the output between poisoned guards: rows of 159 bytes (no
    alignment) and of 192 (the dword path of the vertical kernel); both passes and each alone.  The
    last frame ends at the tensor's last byte, the last table row at the table's."""
    from aiko_services_amd.ops.reference import scale_frames_ref
    from aiko_services_amd.ops.scale import scale_plan
    h, f = 37, "bicubic"
    size = (size[0], size[1] or width)
    frames = S.frames(h, width)
    plan = scale_plan(h, width, size, f, device="cuda")
    fresh = torch.empty(S.B, *size, 3, dtype=torch.uint8, device="cuda")
    torch.ops.aiko.scale_frames_out(frames.cuda(), plan.hb, plan.hk, plan.vb, plan.vk, plan.tile_rows, plan.tile_cols,
                                    plan.win_rows, fresh)
    torch.cuda.synchronize()
    assert torch.equal(fresh.cpu(), scale_frames_ref(frames, size, f))
    gf, cf = guarded(frames.shape, torch.uint8, "cuda", values=frames, name="frames")
    go, co = guarded(fresh.shape, torch.uint8, "cuda", name="out")
    tables, checks = [], [cf, co]
    for name in ("hb", "hk", "vb", "vk"):
        t = getattr(plan, name)
        if t is None:
            tables.append(None)
            continue
        gt, ct = guarded(t.shape, torch.int32, "cuda", values=t, name=name)
        tables.append(gt)
        checks.append(ct)
    torch.ops.aiko.scale_frames_out(gf, *tables, plan.tile_rows, plan.tile_cols, plan.win_rows, go)
    torch.cuda.synchronize()
    for check in checks:
        check()
    assert torch.equal(gf.cpu(), frames)
    for name, gt in zip(("hb", "hk", "vb", "vk"), tables):
        assert gt is None or torch.equal(gt, getattr(plan, name))
    assert torch.equal(go, fresh)


def test_refusals(native):
    from aiko_services_amd.ops.scale import scale_frames, scale_plan
    h, w, ho, wo = 37, 53, 91, 17
    frames = S.frames(h, w).cuda()
    plan = scale_plan(h, w, (ho, wo), "bicubic", device="cuda")

    def op(frames=frames, hb=plan.hb, hk=plan.hk, vb=plan.vb, vk=plan.vk, tile=None, out=None):
        if out is None:
            out = torch.empty(frames.shape[0], ho, wo, 3, dtype=torch.uint8, device="cuda")
        tile = tile or (plan.tile_rows, plan.tile_cols, plan.win_rows)
        torch.ops.aiko.scale_frames_out(frames, hb, hk, vb, vk, *tile, out)

    op()
    wide = torch.zeros(S.B, h, 2 * w, 3, dtype=torch.uint8, device="cuda")
    assert not wide[:, :, ::2].is_contiguous()
    odd = torch.zeros(2 * wo + 1, dtype=torch.int32, device="cuda")[1:].view(wo, 2)        # 4 bytes off 8
    assert odd.data_ptr() % 8 == 4
    for match, kw in [
            ("frames uint8", dict(frames=frames.float())),
            ("frames uint8", dict(frames=frames[..., :2].contiguous())),
            ("frames uint8", dict(frames=frames[0])),
            ("contiguous", dict(frames=wide[:, :, ::2])),
            ("GPU tensor", dict(frames=frames.cpu())),
            ("GPU tensor", dict(hk=plan.hk.cpu())),
            ("GPU tensor", dict(vb=plan.vb.cpu())),
            ("GPU tensor", dict(out=torch.empty(S.B, ho, wo, 3, dtype=torch.uint8))),
            ("out uint8", dict(out=torch.empty(S.B + 1, ho, wo, 3, dtype=torch.uint8, device="cuda"))),
            ("out uint8", dict(out=torch.empty(S.B, ho, wo, 4, dtype=torch.uint8, device="cuda"))),
            ("out uint8", dict(out=torch.empty(S.B, ho, wo, 3, dtype=torch.int8, device="cuda"))),
            ("out uint8", dict(out=torch.empty(S.B, ho, 2 * wo, 3, dtype=torch.uint8, device="cuda")[:, :, ::2])),
            ("horizontal bounds", dict(out=torch.empty(S.B, ho, wo + 1, 3, dtype=torch.uint8, device="cuda"))),
            ("vertical bounds", dict(out=torch.empty(S.B, ho - 1, wo, 3, dtype=torch.uint8, device="cuda"))),
            ("horizontal bounds", dict(hb=plan.hb.long())),
            ("horizontal bounds", dict(hb=plan.hb[:-1])),
            ("horizontal bounds", dict(hb=odd)),
            ("horizontal coefficients", dict(hk=plan.hk.float())),
            ("horizontal coefficients", dict(hk=plan.hk[:, :0])),
            ("horizontal coefficients", dict(hk=plan.hk[:, :-1])),                           # not contiguous
            ("vertical coefficients", dict(vk=plan.vk[:-1])),
            ("together", dict(hb=None)),
            ("together", dict(vk=None)),
            ("keeps that size", dict(hb=None, hk=None)),
            ("keeps that size", dict(vb=None, vk=None)),
            ("a tile of", dict(tile=(0, 64, plan.win_rows))),
            ("a tile of", dict(tile=(ho + 1, 64, plan.win_rows))),
            ("a tile of", dict(tile=(8, 6, plan.win_rows))),
            ("a tile of", dict(tile=(8, 68, plan.win_rows))),
            ("a window of", dict(tile=(8, 64, 0))),
            ("a window of", dict(tile=(8, 64, h + 1)))]:
        with pytest.raises(RuntimeError, match=match):
            op(**kw)
    with pytest.raises(RuntimeError, match="no pass to run"):
        op(hb=None, hk=None, vb=None, vk=None, out=torch.empty_like(frames))
    tall = torch.zeros(1, 1000, 8, 3, dtype=torch.uint8, device="cuda")
    tall_plan = scale_plan(1000, 8, (2, 4), "box", device="cuda")
    with pytest.raises(RuntimeError, match="a window of"):                                   # 192 KB of LDS
        op(frames=tall, hb=tall_plan.hb, hk=tall_plan.hk, vb=tall_plan.vb, vk=tall_plan.vk, tile=(2, 64, 1000),
           out=torch.empty(1, 2, 4, 3, dtype=torch.uint8, device="cuda"))
    # an output that overlaps the frames
    n_out = S.B * ho * wo * 3
    big = torch.zeros(2 * max(frames.numel(), n_out), dtype=torch.uint8, device="cuda")
    inside = big[:frames.numel()].view(frames.shape)
    with pytest.raises(RuntimeError, match="out and frames overlap"):
        op(frames=inside, out=big[frames.numel() - 3:][:n_out].view(S.B, ho, wo, 3))
    op(frames=inside, out=big[frames.numel():][:n_out].view(S.B, ho, wo, 3))                 # adjacent: fine
    # ... or a table: the coefficients as an int32 view of the bytes in front of out
    nk = plan.vk.numel() * 4
    raw = torch.zeros(nk + n_out, dtype=torch.uint8, device="cuda")
    vk_inside = raw[:nk].view(torch.int32).view(plan.vk.shape)
    vk_inside.copy_(plan.vk)
    with pytest.raises(RuntimeError, match="out and the vertical coefficients overlap"):
        op(vk=vk_inside, out=raw[nk - 4:][:n_out].view(S.B, ho, wo, 3))
    op(vk=vk_inside, out=raw[nk:].view(S.B, ho, wo, 3))                                      # adjacent: fine
    # the front end's own checks
    for match, args, kw in [("filter", ((ho, wo), "cubic"), {}), ("sizes", ((0, wo),), {}), ("size =", (ho,), {}),
                            ("outside the frame", ((ho, wo),), dict(box=(0, 0, 16 * w + 1, 16 * h))),
                            ("integer", ((ho, wo),), dict(box=(0, 0, 8.5, 16 * h))),
                            ("frames uint8", None, {}), ("out uint8", ((h, w),), dict(out=torch.empty(1, device="cuda")))]:
        with pytest.raises(ValueError, match=match):
            if args is None:
                scale_frames(frames[0], (ho, wo))
            else:
                scale_frames(frames, *args, **kw)
    same = scale_frames(frames, (h, w))                      # the same size with no box: a copy
    assert torch.equal(same, frames) and same.data_ptr() != frames.data_ptr()
    torch.cuda.synchronize()


# ---- ImageResize and the example pipeline -----------------------------------------------------

def _create(d):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<scale>", parse_pipeline_definition_dict(d), None, None, "c", [], 0, None, 60,
                                     queue_response=q)
    p.response_swag = True                     # the whole swag comes back, device tensors included
    return p, q


def test_image_resize_device_branch_equals_host_branch(native):
    from aiko_services_amd.ops.reference import scale_frames_ref
    from aiko_services_amd.ops.vision import resize_u8
    from aiko_services_amd.pipeline.stream import StreamEvent

    def element(**parameters):
        d = {"version": 0, "name": "p_resize", "runtime": "python", "graph": ["(ImageResize)"], "parameters": {},
             "elements": [{"name": "ImageResize", "input": [{"name": "images", "type": "[image]"}],
                           "output": [{"name": "images", "type": "[image]"}], "parameters": parameters,
                           "deploy": {"local": {"module": "aiko_services_amd.elements.media.image_io"}}}]}
        return _create(d)[0].pipeline_graph.get_node("ImageResize").element

    frames = S.frames(37, 53)
    for name in ("bicubic", "lanczos", "box"):
        resize = element(resolution="17x91", filter=name)
        event, device = resize.process_frame(None, frames.cuda())
        assert event == StreamEvent.OKAY and device["images"].is_cuda
        torch.cuda.synchronize()
        event, host = resize.process_frame(None, [f.numpy() for f in frames])       # the downloaded frames
        assert event == StreamEvent.OKAY
        assert np.array_equal(device["images"].cpu().numpy(), np.stack(host["images"])), name
        assert torch.equal(device["images"].cpu(), scale_frames_ref(frames, (91, 17), name))
    # without ``filter`` the device branch is the two-tap kernel it was
    event, out = element(resolution="17x91").process_frame(None, frames.cuda())
    torch.cuda.synchronize()
    assert event == StreamEvent.OKAY and torch.equal(out["images"], resize_u8(frames.cuda(), (91, 17)))
    event, out = element(resolution="17x91", filter="nearest").process_frame(None, frames.cuda())
    assert event == StreamEvent.ERROR and "filter" in out["diagnostic"]


# conf 0.2987 on 240 x 320 noise frames keeps 1-3 boxes per frame of the seeded YOLOv8-n
# (test_gpu_roi.py), so the frames FrameScale reduces carry drawn boxes and labels
PIPE_B, PIPE_H, PIPE_W = 2, 240, 320
PIPE_CONF = 0.2987
PIPE_FRAMES = 3
EXAMPLE = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/yolo/yolo_thumbnail_gpu.json"


def _definition(lanes=1, **scale_parameters):
    d = json.loads(EXAMPLE.read_text())
    assert d["graph"] == ["(SyntheticFrames YoloDetector DetectionOverlay FrameScale JpegEncode JpegResults)"]
    d["parameters"]["gpu_lanes"] = lanes
    by_name = {e["name"]: e for e in d["elements"]}
    source = by_name["SyntheticFrames"]["parameters"]
    scale = by_name["FrameScale"]["parameters"]
    assert (scale["height"], scale["width"]) == (source["height"] // 4, source["width"] // 4)   # a quarter-size frame
    source.update(batch=PIPE_B, height=PIPE_H, width=PIPE_W)
    by_name["YoloDetector"]["parameters"].update(autotune=False, graph=True, conf=PIPE_CONF)
    scale.update(height=PIPE_H // 4, width=PIPE_W // 4)
    scale.update(scale_parameters)
    return d


def _run_pipeline(lanes, **scale_parameters):
    p, q = _create(_definition(lanes, **scale_parameters))
    # JpegEncode replaces ``images`` in the swag: keep what the element was given and what it gave
    element = p.pipeline_graph.get_node("FrameScale").element
    inner, seen = element.process_frame, []

    def spy(stream, images):
        event, result = inner(stream, images)
        seen.append({"frames": images.clone(), "scaled": result["images"].clone()})
        return event, result

    element.process_frame = spy
    for i in range(PIPE_FRAMES):
        p.process_frame({"stream_id": "c", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        torch.cuda.synchronize()               # buffers are reused per lane: copy before the next frame
        assert swag["format"] == "jpeg" and len(swag["images"]) == PIPE_B
        assert all(bytes(image[:2]) == b"\xff\xd8" for image in swag["images"])
    assert p.share["gpu_lanes"] == lanes and len(seen) == PIPE_FRAMES
    return seen, element


def test_thumbnail_pipeline_matches_direct_calls(native):
    from aiko_services_amd.ops.reference import scale_frames_ref
    from aiko_services_amd.ops.scale import scale_frames
    size = (PIPE_H // 4, PIPE_W // 4)
    one, element = _run_pipeline(1)
    assert element.filter == "bicubic" and element.box is None
    for i, o in enumerate(one):
        assert o["scaled"].shape == (PIPE_B, *size, 3)
        direct = scale_frames(o["frames"], size, "bicubic")
        torch.cuda.synchronize()
        assert torch.equal(o["scaled"], direct), i
        assert torch.equal(o["scaled"].cpu(), scale_frames_ref(o["frames"], size, "bicubic")), i
    assert not torch.equal(one[0]["frames"], one[1]["frames"])
    two, _ = _run_pipeline(2)
    for a, b in zip(one, two):
        assert torch.equal(a["frames"], b["frames"]) and torch.equal(a["scaled"], b["scaled"])
    # a box given in pixels as JSON text: a digital zoom into the frame
    zoom, element = _run_pipeline(1, filter="lanczos", box="[40.25, 30, 280, 209.5]")
    assert element.box == (644, 480, 4480, 3352)
    for o in zoom:
        assert torch.equal(o["scaled"].cpu(), scale_frames_ref(o["frames"], size, "lanczos", element.box))


def test_frame_scale_diagnostics_and_parameters(native):
    from aiko_services_amd.pipeline.stream import StreamEvent

    def make(**params):                          # the element alone behind a frame source
        d = _definition(1, **params)
        d["graph"] = ["(SyntheticFrames FrameScale)"]
        d["elements"] = [e for e in d["elements"] if e["name"] in ("SyntheticFrames", "FrameScale")]
        return _create(d)[0].pipeline_graph.get_node("FrameScale").element

    for params in (dict(width=0), dict(height=-3), dict(width="wide"), dict(filter="cubic"), dict(box="[0, 0, 10]"),
                   dict(box="[0, 0, 10.03, 10]"), dict(box="0, 0, 10, 10"), dict(box="[0, 0, \"a\", 10]")):
        with pytest.raises(ValueError, match="FrameScale"):
            make(**params)
    d = _definition(1)
    del {e["name"]: e for e in d["elements"]}["FrameScale"]["parameters"]["width"]
    d["graph"] = ["(SyntheticFrames FrameScale)"]
    d["elements"] = [e for e in d["elements"] if e["name"] in ("SyntheticFrames", "FrameScale")]
    with pytest.raises(ValueError, match="width and height are required"):
        _create(d)
    element = make(box="[0, 0, 320, 240]")
    good = torch.zeros(PIPE_B, PIPE_H, PIPE_W, 3, dtype=torch.uint8, device="cuda")
    event, out = element.process_frame(None, good)
    assert event == StreamEvent.OKAY and out["images"].shape == (PIPE_B, PIPE_H // 4, PIPE_W // 4, 3)
    again = element.process_frame(None, good)[1]["images"]
    assert again.data_ptr() == out["images"].data_ptr()                        # one buffer per (shape, lane)
    for args, text in (((good.float(),), "images uint8"), ((good[..., :2],), "images uint8"),
                       ((good.cpu(),), "images uint8"), ((None,), "images uint8"),
                       ((good[:, :100].contiguous(),), "outside the frame")):  # the box is 240 rows high
        event, out = element.process_frame(None, *args)
        assert event == StreamEvent.ERROR and "FrameScale" in out["diagnostic"] and text in out["diagnostic"], out
    event, out = make().process_frame(None, torch.zeros(1, 8, 300000, 3, dtype=torch.uint8, device="cuda"))
    assert event == StreamEvent.ERROR and "MAX_TAPS" in out["diagnostic"]
    # the same size with no box passes the batch through
    same = make(height=PIPE_H, width=PIPE_W)
    event, out = same.process_frame(None, good)
    assert event == StreamEvent.OKAY and out["images"] is good
    torch.cuda.synchronize()
