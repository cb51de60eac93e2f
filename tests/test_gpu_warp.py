"""The warp kernel (``ops.warp.warp_quads``, warp_ops.hip) against ``warp_quads_ref``, bit for bit: the
marker scenes' quads and random ones at both frame widths, small, oblong, wide and whole-frame patches,
unused slots of every kind; the six views against torch's flips and turns; between guard bands; under
hipGraph replay; the operator's refusals; then ``QuadRectify`` behind ``MarkerDetector`` and
``FrameWarp`` in pipelines."""
import json
import queue
from pathlib import Path

import numpy as np
import pytest
import torch

import marker_scenes as S
import warp_scenes as WS
from kernel_guard import guarded
from warp_scenes import B, H

pytestmark = pytest.mark.gpu

EXAMPLES = Path(__file__).resolve().parents[1] / "aiko_services_amd" / "examples"


def _case(case, width):
    return WS.random_case(width) if case == "random" else WS.marker_case(case, width)[:3]


def _run(frames, quads, count, k, size, margin=0, origin="centre"):
    """The kernel on fresh device tensors, the outputs pre-filled: every element must be rewritten."""
    from aiko_services_amd.ops.warp import warp_quads
    patches = torch.full((frames.shape[0] * k, *size, 3), 0xFF, dtype=torch.uint8, device="cuda")
    valid = torch.full((frames.shape[0] * k,), -1, dtype=torch.int32, device="cuda")
    got = warp_quads(frames.cuda(), quads.cuda(), count.cuda(), k, size, margin, origin, patches=patches, valid=valid)
    torch.cuda.synchronize()
    assert got[0] is patches and got[1] is valid
    return patches.cpu(), valid.cpu()


def _assert_equal(got, want, where):
    assert got[1].dtype == torch.int32 and torch.equal(got[1], want[1]), f"{where}: valid {got[1]} != {want[1]}"
    assert got[0].dtype == torch.uint8 and got[0].shape == want[0].shape
    if not torch.equal(got[0], want[0]):
        diff = (got[0] != want[0]).nonzero()
        at = tuple(diff[0].tolist())
        raise AssertionError(f"{where}: {len(diff)} bytes differ, the first at {at}: {int(got[0][at])} != {int(want[0][at])}")


# k of 1, 4 and 16 with Kq > k (16 rows of marker corners, 20 random quads); 8 x 8, 56 x 56 and 36 x 60
# patches; both widths; margins on both sides of the horizon quad's horizon (slot 4 of the random case)
CASES = [("large", S.W, 4, (56, 56), 0), ("angles_a", S.W_ODD, 4, (56, 56), 2), ("angles_b", S.W, 1, (8, 8), 8),
         ("upright", S.W_ODD, 4, (36, 60), 0), ("random", S.W, 16, (56, 56), 0), ("random", S.W_ODD, 16, (36, 60), 64),
         ("random", S.W_ODD, 4, (8, 8), 5), ("random", S.W, 1, (36, 60), 3)]


@pytest.mark.parametrize("case,width,k,size,margin", CASES)
def test_patches_equal_reference(native, case, width, k, size, margin):
    frames, quads, count = _case(case, width)
    assert quads.shape[1] > k
    want = WS.reference(case, width, k, size, margin)
    _assert_equal(_run(frames, quads, count, k, size, margin), want, f"{case}, width {width}, k {k}, {size}, m {margin}")
    if case == "random" and k == 16:
        # frame 0 has count 0, frame 1 seven rows with the three unused kinds at 1..3, frame 2 more than k
        assert want[1].tolist() == [0] * 16 + [1, 0, 0, 0, 1, 1, 1] + [0] * 9 + [1, 0, 0, 0] + [1] * 12
        assert not want[0][:16].any() and want[0][16].any()
        if margin == 64:                                       # the horizon quad: zero pixels and others
            assert (want[0][20] == 0).all(-1).any() and want[0][20].any()


@pytest.mark.parametrize("width", S.WIDTHS)
def test_whole_frame_and_wide_patches(native, width):
    """176 x 208 patches are five bands of 32 rows and one of 16; 40 x 320 patches are one chunk of 64
    lanes and one of 16 per row."""
    frames = WS.noise(H, width, seed=9, b=B)
    keystone = [[(10, 4), (width - 3, 20), (width + 12, H - 9), (-6, H + 2)],
                [(width, 0), (0, 0), (20, H), (width - 20, H)], [(0, 0), (width, 0), (width, H), (0, H)]]
    quads = torch.tensor(keystone, dtype=torch.int32).view(B, 1, 4, 2).repeat(1, 2, 1, 1)
    count = torch.ones(B, dtype=torch.int32)
    from aiko_services_amd.ops.reference import warp_quads_ref
    for size, origin in (((176, 208), "edge"), ((40, 320), "centre"), ((33, 4), "edge")):
        want = warp_quads_ref(frames, quads, count, 1, size, 0, origin)
        _assert_equal(_run(frames, quads, count, 1, size, 0, origin), want, f"width {width}, {size}, {origin}")
        assert want[1].tolist() == [1] * B and all(p.any() for p in want[0])


def test_six_views_equal_torch(native):
    from aiko_services_amd.ops.warp import VIEWS
    frames = WS.noise(H, S.W, seed=4, b=B)
    dev = frames.cuda()
    want = {"identity": dev, "flip_h": dev.flip(2), "flip_v": dev.flip(1), "rot180": dev.flip(1, 2),
            "rot90": torch.rot90(dev, -1, (1, 2)), "rot270": torch.rot90(dev, 1, (1, 2))}
    assert sorted(want) == sorted(VIEWS)
    for name in VIEWS:
        quads, count, size = WS.view_case(name, H, S.W, b=B)
        patches, valid = _run(frames, quads, count, 1, size, 0, "edge")
        assert valid.tolist() == [1] * B and tuple(patches.shape) == (B, *size, 3)
        assert torch.equal(patches, want[name].contiguous().cpu()), name
    assert want["rot90"].shape == (B, S.W, H, 3) and torch.equal(want["rot90"][0, 0, 0], dev[0, H - 1, 0])


@pytest.mark.parametrize("width,k,size,margin", [(S.W_ODD, 16, (36, 60), 5), (S.W, 4, (56, 56), 0)])
def test_guard_bands_and_no_poison_left(native, width, k, size, margin):
    from aiko_services_amd.ops.warp import warp_quads
    frames, quads, count = WS.random_case(width)
    checks = []

    def g(shape, dtype, label, values=None):
        view, check = guarded(shape, dtype, "cuda", values=values, name=label)
        checks.append(check)
        return view

    gf, gq, gc = g(frames.shape, torch.uint8, "frames", frames), g(quads.shape, torch.int32, "quads", quads), \
        g(count.shape, torch.int32, "count", count)
    gp, gv = g((B * k, *size, 3), torch.uint8, "patches"), g((B * k,), torch.int32, "valid")
    warp_quads(gf, gq, gc, k, size, margin, patches=gp, valid=gv)
    torch.cuda.synchronize()
    for check in checks:
        check()
    _assert_equal((gp.cpu(), gv.cpu()), WS.reference("random", width, k, size, margin), "guarded")
    _assert_equal((gp.cpu(), gv.cpu()), _run(frames, quads, count, k, size, margin), "guarded against fresh tensors")
    # no slot kept its poison, the unused ones included; the inputs are only read
    assert not (gp.view(B * k, -1) == 0xA5).all(1).any() and bool(((gv == 0) | (gv == 1)).all())
    assert torch.equal(gf.cpu(), frames) and torch.equal(gq.cpu(), quads) and torch.equal(gc.cpu(), count)
    if k == 16:
        # the largest used quad (slot 5 of the last frame) ends at the frame's last pixel, the tensor's
        # last three bytes, right in front of the guard
        assert torch.equal(gp[2 * k + 5, -1, -1].cpu(), frames[2, -1, -1])


def test_rows_past_count_are_never_read(native):
    frames, quads, count = WS.random_case(S.W)
    base = _run(frames, quads, count, 16, (8, 8))
    q = quads.clone()
    q[0] = 2 ** 31 - 1                                       # count 0
    q[1, 7:] = -2 ** 31                                      # count 7
    _assert_equal(_run(frames, q, count, 16, (8, 8)), base, "garbage past the count")


def test_quads_and_count_are_read_at_graph_replay(native):
    from aiko_services_amd.ops.reference import warp_quads_ref
    from aiko_services_amd.ops.warp import warp_quads
    k, size, margin = 4, (36, 60), 3
    first, other = WS.random_case(S.W_ODD), WS.random_case(S.W_ODD, seed=8)
    frames, quads, count = (t.cuda() for t in first)
    patches = torch.empty(B * k, *size, 3, dtype=torch.uint8, device="cuda")
    valid = torch.empty(B * k, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warp_quads(frames, quads, count, k, size, margin, patches=patches, valid=valid)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        warp_quads(frames, quads, count, k, size, margin, patches=patches, valid=valid)
    seen = []
    for step, (new_quads, new_count) in enumerate([(first[1], first[2]), (other[1], torch.tensor([3, 0, 1])),
                                                   (other[1].flip(0), torch.tensor([-5, 2, 9]))]):
        new_count = new_count.to(torch.int32)
        quads.copy_(new_quads)
        count.copy_(new_count)
        patches.fill_(0x5A)
        valid.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal((patches.cpu(), valid.cpu()), warp_quads_ref(first[0], new_quads, new_count, k, size, margin),
                      f"replay {step}")
        seen.append(valid.cpu().clone())
    assert (seen[1] & ~seen[0]).any() and (seen[0] & ~seen[1]).any()           # slots flipped both ways


def test_refusals(native):
    from aiko_services_amd.ops.warp import warp_quads
    frames, quads, count = (t.cuda() for t in WS.random_case(S.W))
    kq, dev, i32, u8 = quads.shape[1], "cuda", torch.int32, torch.uint8

    def refuse(match, error=RuntimeError, k=4, size=(8, 8), **kw):
        args = {**dict(frames=frames, quads=quads, count=count), **kw}
        with pytest.raises(error, match=match):
            warp_quads(args.pop("frames"), args.pop("quads"), args.pop("count"), k, size, **args)

    # dtypes, shapes, contiguity
    refuse("frames uint8", frames=frames.float())
    refuse("frames uint8", frames=frames[..., :2].contiguous())
    refuse("frames uint8", frames=torch.zeros(B, H, 2 * S.W, 3, dtype=u8, device=dev)[:, :, ::2])
    refuse("frames uint8", frames=torch.zeros(1, 1, 1, 3, dtype=u8, device=dev), quads=quads[:1], count=count[:1])
    refuse("quads int32", quads=quads.float())
    refuse("quads int32", quads=quads[:2])
    refuse("quads int32", quads=quads.view(B, kq, 8))
    refuse("quads int32", quads=torch.zeros(B, 2 * kq, 4, 2, dtype=i32, device=dev)[:, ::2])
    refuse("count int32", count=count.long())
    refuse("count int32", count=torch.zeros(B + 1, dtype=i32, device=dev))
    refuse("count int32", count=torch.zeros(2 * B, dtype=i32, device=dev)[::2])
    refuse("patches uint8", patches=torch.empty(B * 4, 8, 8, 3, dtype=torch.int8, device=dev))
    refuse("patches uint8", patches=torch.empty(B * 4 + 1, 8, 8, 3, dtype=u8, device=dev))
    refuse("patches uint8", patches=torch.empty(B * 4, 8, 8, 4, dtype=u8, device=dev))
    refuse("patches uint8", patches=torch.empty(B * 4, 8, 16, 3, dtype=u8, device=dev)[:, :, ::2])
    refuse("valid int32", valid=torch.empty(B * 4, dtype=torch.float32, device=dev))
    refuse("valid int32", valid=torch.empty(B * 4 + 1, dtype=i32, device=dev))
    refuse("valid int32", valid=torch.empty(B * 8, dtype=i32, device=dev)[::2])
    # devices
    refuse("GPU tensor", frames=frames.cpu(), patches=torch.empty(B * 4, 8, 8, 3, dtype=u8, device=dev))
    refuse("GPU tensor", quads=quads.cpu())
    refuse("GPU tensor", count=count.cpu())
    refuse("GPU tensor", valid=torch.empty(B * 4, dtype=i32))
    if torch.cuda.device_count() > 1:
        refuse("device", count=count.to("cuda:1"))
    # overlap of an output with an input or the other output
    refuse("patches and frames overlap", patches=frames.view(-1)[:B * 4 * 8 * 8 * 3].view(B * 4, 8, 8, 3))
    refuse("valid and quads overlap", valid=quads.view(-1)[:B * 4])
    refuse("valid and count overlap", k=1, valid=count)
    both = torch.zeros(B * 4 * 8 * 8 * 3 // 4 + B * 4, dtype=i32, device=dev)
    refuse("valid and patches overlap", patches=both.view(u8)[:B * 4 * 8 * 8 * 3].view(B * 4, 8, 8, 3), valid=both[8:8 + B * 4])
    # misaligned patches (an int32 tensor cannot be misaligned)
    raw = torch.zeros(B * 4 * 8 * 8 * 3 + 4, dtype=u8, device=dev)
    for shift in (1, 2, 3):
        refuse("4-byte aligned", patches=raw[shift:shift + B * 4 * 8 * 8 * 3].view(B * 4, 8, 8, 3))
    # values: Python errors first, then the operator's own bounds past the Python layer
    refuse("multiple of 4", error=ValueError, size=(8, 10))
    refuse("Ho, Wo", error=ValueError, size=(4097, 8))
    refuse("margin", error=ValueError, margin=65)
    refuse("origin", error=ValueError, origin="middle")
    refuse("k <= Kq", k=kq + 1)
    patches, valid = torch.empty(B * 4, 8, 8, 3, dtype=u8, device=dev), torch.empty(B * 4, dtype=i32, device=dev)
    op = torch.ops.aiko.quad_warp_out
    for bad, match in (((0, 0, 1), "k <= Kq"), ((4, -1, 1), "margin"), ((4, 65, 1), "margin"), ((4, 0, 2), "origin")):
        with pytest.raises(RuntimeError, match=match):
            op(frames, quads, count, *bad, patches, valid)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        op(frames, quads, count, 4, 0, 1, torch.empty(B * 4, 8, 10, 3, dtype=u8, device=dev), valid)
    with pytest.raises(RuntimeError, match="patch side <= 4096"):
        op(frames[:1], quads[:1], count[:1], 1, 0, 1, torch.empty(1, 1, 4100, 3, dtype=u8, device=dev), valid[:1])
    with pytest.raises(RuntimeError, match="patch side <= 4096"):
        op(frames[:1], quads[:1], count[:1], 1, 0, 1, torch.empty(1, 4097, 4, 3, dtype=u8, device=dev), valid[:1])
    for shape in ((1, 2, 4097, 3), (1, 4097, 2, 3)):
        with pytest.raises(RuntimeError, match="exceed the frame limit"):
            op(torch.zeros(shape, dtype=u8, device=dev), quads[:1], count[:1], 4, 0, 1, patches[:4], valid[:4])
    # B * k above the grid limit
    many = 16384
    with pytest.raises(RuntimeError, match="exceed the grid limit"):
        op(torch.zeros(many, 2, 2, 3, dtype=u8, device=dev), torch.zeros(many, 4, 4, 2, dtype=i32, device=dev),
           torch.zeros(many, dtype=i32, device=dev), 4, 0, 1, torch.empty(many * 4, 1, 4, 3, dtype=u8, device=dev),
           torch.empty(many * 4, dtype=i32, device=dev))
    # inside the limits: 4096 pixels a side both ways, one quad
    big = torch.full((1, 2, 4096, 3), 200, dtype=u8, device=dev)
    q, size = WS.view_case("identity", 2, 4096)[0].cuda(), (2, 4096)
    out, ok = warp_quads(big, q, count[:1].fill_(1), 1, size, 0, "edge")
    torch.cuda.synchronize()
    assert ok.tolist() == [1] and torch.equal(out, big)


# ---- the elements ---------------------------------------------------------------------------

PIPE_SCENE, PIPE_FRAMES, PIPE_QUADS, PIPE_SIZE, PIPE_MARGIN = "large", 3, 4, 112, 8


def _pipeline(definition, lanes, height=H, width=S.W):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    definition["parameters"]["gpu_lanes"] = lanes
    by_name = {e["name"]: e for e in definition["elements"]}
    by_name["SyntheticFrames"]["parameters"].update(batch=B, height=height, width=width, pool=1)
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<warp>", parse_pipeline_definition_dict(definition), None, None, "c", [], 0, None,
                                     60, queue_response=q)
    p.response_swag = True                     # the whole swag comes back, device tensors included
    source = p.pipeline_graph.get_node("SyntheticFrames").element
    source._ensure_pool(False)
    return p, q, source


def _rectify_outputs(lanes):
    d = json.loads((EXAMPLES / "aruco_marker" / "aruco_rectify_gpu.json").read_text())
    {e["name"]: e for e in d["elements"]}["QuadRectify"]["parameters"].update(quads=PIPE_QUADS, image_size=PIPE_SIZE,
                                                                               margin=PIPE_MARGIN)
    p, q, source = _pipeline(d, lanes)
    source.frame_pool.view(0, source._shape, torch.uint8).copy_(S.scene(PIPE_SCENE).frames)
    torch.cuda.synchronize()
    outs = []
    for i in range(PIPE_FRAMES):
        p.process_frame({"stream_id": "c", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        torch.cuda.synchronize()               # buffers are reused per lane: copy before the next frame
        crops = swag["JpegEncode.images"]      # the (crops: images) mapping files the crops under the consumer's name
        outs.append({"crops": crops.clone(), "valid": swag["crops_valid"].clone(), "counts": swag["counts"].clone(),
                     "jpeg": [x.tobytes() for x in swag["images"]], "address": crops.data_ptr()})
    assert p.share["gpu_lanes"] == lanes
    return outs


def test_quad_rectify_behind_marker_detector(native):
    _, _, count, ids = WS.marker_case(PIPE_SCENE)
    want = WS.reference(PIPE_SCENE, S.W, PIPE_QUADS, (PIPE_SIZE, PIPE_SIZE), PIPE_MARGIN)
    one, two = _rectify_outputs(1), _rectify_outputs(2)
    assert len({o["address"] for o in one}) == 1 and len({o["address"] for o in two}) <= 2     # a buffer pair per lane
    read = 0
    for o in one + two:
        assert o["counts"].tolist() == count.tolist() and tuple(o["crops"].shape) == (B * PIPE_QUADS, PIPE_SIZE, PIPE_SIZE, 3)
        assert o["valid"].tolist() == [int(i < min(int(count[b]), PIPE_QUADS)) for b in range(B) for i in range(PIPE_QUADS)]
        _assert_equal((o["crops"].cpu(), o["valid"].cpu()), want, "pipeline")
        for b in range(B):
            for i in range(min(int(count[b]), PIPE_QUADS)):
                got = WS.read_modules(o["crops"][b * PIPE_QUADS + i].cpu(), 7, PIPE_MARGIN)
                assert np.array_equal(got, S.module_grid("original", int(ids[b, i]))), (b, i)
                read += 1
        assert len(o["jpeg"]) == B * PIPE_QUADS and all(j[:2] == b"\xff\xd8" and j[-2:] == b"\xff\xd9" for j in o["jpeg"])
    assert read == 6 * 2 * PIPE_FRAMES


def _frame_warp(view, size=None, height=H, width=S.W):
    d = json.loads((EXAMPLES / "yolo" / "yolo_rot180_gpu.json").read_text())
    d["graph"] = ["(SyntheticFrames FrameWarp)"]
    d["elements"] = [e for e in d["elements"] if e["name"] in ("SyntheticFrames", "FrameWarp")]
    d["elements"][1]["parameters"] = {"view": view, **({} if size is None else {"size": size})}
    return _pipeline(d, 1, height, width)


def test_frame_warp(native):
    from aiko_services_amd.ops.reference import warp_quads_ref
    from aiko_services_amd.pipeline.stream import StreamEvent
    # the example's own view first, then a quarter turn: through the pipeline
    for view, turn in (("rot180", lambda x: x.flip(1, 2)), ("rot90", lambda x: torch.rot90(x, -1, (1, 2)))):
        p, q, source = _frame_warp(view)
        frames = source.frame_pool.view(0, source._shape, torch.uint8).clone()
        p.process_frame({"stream_id": "c", "frame_id": 0}, {})
        info, swag = q.get_nowait()
        torch.cuda.synchronize()
        assert info["state"] == 0, swag
        assert tuple(swag["images"].shape) == ((B, S.W, H, 3) if view == "rot90" else (B, H, S.W, 3))
        assert torch.equal(swag["images"], turn(frames).contiguous()), view
    # a width that is no multiple of 4 is an ERROR event that says so: the quarter turn of 176 x 203
    # frames (H x W) is 176 wide and fine, that of 203 x 176 frames is 203 wide
    element = p.pipeline_graph.get_node("FrameWarp").element
    odd = WS.noise(H, S.W_ODD, b=B).cuda()
    event, out = element.process_frame(None, odd)
    torch.cuda.synchronize()
    assert event == StreamEvent.OKAY and torch.equal(out["images"], torch.rot90(odd, -1, (1, 2)).contiguous())
    event, out = element.process_frame(None, WS.noise(S.W_ODD, H, b=B).cuda())
    assert event == StreamEvent.ERROR and "multiple of 4" in out["diagnostic"], out
    for bad in (odd.float(), odd.cpu(), odd[..., :2], None):
        event, out = element.process_frame(None, bad)
        assert event == StreamEvent.ERROR and "images uint8" in out["diagnostic"], out
    # one view per camera, at a size of its own: row b gets quad b
    views = [[0, 0, S.W, 0, S.W, H, 0, H], [S.W, H, 0, H, 0, 0, S.W, 0], [30, 10, 190, 25, 170, 160, 12, 140]]
    p, q, source = _frame_warp(json.dumps(views), size="[96, 120]")    # element parameters are scalars: JSON text
    element = p.pipeline_graph.get_node("FrameWarp").element
    frames = WS.noise(H, S.W, seed=2, b=B)
    event, out = element.process_frame(None, frames.cuda())
    torch.cuda.synchronize()
    quads = torch.tensor(views, dtype=torch.int32).view(B, 1, 4, 2)
    want = warp_quads_ref(frames, quads, torch.ones(B, dtype=torch.int32), 1, (96, 120), 0, "edge")[0]
    assert event == StreamEvent.OKAY and torch.equal(out["images"].cpu(), want)
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])
    event, out = element.process_frame(None, frames[:2].cuda())         # three cameras listed, two frames
    assert event == StreamEvent.ERROR and "cameras" in out["diagnostic"], out


def test_quad_rectify_diagnostics(native):
    from aiko_services_amd.pipeline.stream import StreamEvent
    d = json.loads((EXAMPLES / "aruco_marker" / "aruco_rectify_gpu.json").read_text())
    p, q, source = _pipeline(d, 1)
    element = p.pipeline_graph.get_node("QuadRectify").element
    frames, corners, count, _ = WS.marker_case("upright")
    good = (frames.cuda(), corners.cuda(), count.cuda())
    event, out = element.process_frame(None, *good)
    torch.cuda.synchronize()
    assert event == StreamEvent.OKAY and out["images"] is good[0] and out["counts"] is good[2]
    assert out["crops"].shape == (B * 4, 224, 224, 3) and out["crops_valid"].tolist() == [1] * 4 + [1, 0, 0, 0] + [0] * 4
    for bad, text in (((good[0].float(), good[1], good[2]), "images uint8"), ((good[0].cpu(), good[1], good[2]), "images uint8"),
                      ((None, good[1], good[2]), "images uint8"), ((good[0], good[1].float(), good[2]), "marker_corners int32"),
                      ((good[0], good[1][:, :3], good[2]), "marker_corners int32"), ((good[0], good[1][:2], good[2]), "marker_corners int32"),
                      ((good[0], None, good[2]), "marker_corners int32"), ((good[0], good[1], good[2].long()), "counts int32"),
                      ((good[0], good[1], good[2][:2]), "counts int32"), ((good[0], good[1], good[2].cpu()), "counts int32")):
        event, out = element.process_frame(None, *bad)
        assert event == StreamEvent.ERROR and text in out["diagnostic"], out
    torch.cuda.synchronize()
