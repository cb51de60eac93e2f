"""The camera wall on the MI355X (``wall_ops.hip``): wall and source bit for bit against
``frame_wall_ref`` on the shared scenes (wall_scenes.py) in both orders with ring and label on and
off, the path without a score, device-side scores and frames under hipGraph replay, guard bands,
cameras that are not shown, refusals, and the FrameWall element in its example pipeline against the
same kernels called directly."""
import json
import queue
from pathlib import Path

import pytest
import torch

import wall_scenes as S
from kernel_guard import guarded

pytestmark = pytest.mark.gpu


def run(case, order="index", opt=0, score=True, frames=None, **kw):
    from aiko_services_amd.ops.wall import frame_wall
    h, w, tile = case
    frames = S.frames(h, w) if frames is None else frames
    args = dict(rows=S.ROWS, cols=S.COLS, tile=tile, pages=S.PAGES, order=order, **S.options(case, opt), **S.COLOURS)
    args.update(kw)
    wall, source = frame_wall(frames.cuda(), S.scores().cuda() if score is True else score, **args)
    torch.cuda.synchronize()
    return wall.cpu(), source.cpu()


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_equals_reference(native, case):
    before = S.frames(case[0], case[1]).clone()
    for order in ("index", "score"):
        for opt in range(len(S.OPTIONS)):
            wall, source = run(case, order, opt)
            ref_wall, ref_source = S.reference(case, order, opt)
            diff = (wall != ref_wall).any(-1)
            print(f"wall {S.case_id(case)} {order} options {opt}: {int(diff.sum())} of {diff.numel()} pixels differ "
                  f"{torch.nonzero(diff)[:5].tolist()}, source {source.tolist()}")
            assert torch.equal(source, ref_source)
            assert torch.equal(wall, ref_wall)
    assert ref_source.view(-1)[:5].tolist() == S.SCORE_ORDER + [-1]
    assert torch.equal(S.frames(case[0], case[1]), before)


def test_positions_past_32_bits(native):
    """A 70000-pixel row reduced to 65000: tw * W is past 2^32, the kernel's other way to a
    footprint's first column.  ``frame_wall_ref``'s dense weights would be 36 GB here, so the
    expected row comes from the rule's sum over the at most three source columns of a pixel."""
    import numpy as np
    from aiko_services_amd.ops.wall import frame_wall
    W, tw = 70000, 65000
    assert tw * W > 2 ** 32 and W % 16 == 0
    g = torch.Generator().manual_seed(7)
    frames = torch.randint(0, 256, (2, 1, W, 3), dtype=torch.uint8, generator=g)
    wall, source = frame_wall(frames.cuda(), rows=1, cols=1, tile=(1, tw), pages=2)
    torch.cuda.synchronize()
    assert source.view(-1).tolist() == [0, 1]
    x = np.arange(tw, dtype=np.int64)
    j0 = x * W // tw
    r = x * W - j0 * tw
    for cam in range(2):
        p = frames[cam, 0].numpy().astype(np.int64)
        S_ = np.zeros((tw, 3), np.int64)
        total = np.zeros(tw, np.int64)
        for k in range(3):
            w = np.maximum(0, np.minimum((k + 1) * tw, r + W) - np.maximum(k * tw, r))
            S_ += w[:, None] * p[np.minimum(j0 + k, W - 1)]
            total += w
        assert (total == W).all()
        assert np.array_equal(wall[cam, 0].cpu().numpy(), (2 * S_ + W) // (2 * W))


def test_without_a_score(native):
    """No score: index order, and no tile is ringed whatever ``ring`` says."""
    case = S.CASES[0]
    wall, source = run(case, "index", 1, score=None)
    ref_wall, ref_source = S.reference(case, "index", 1, with_score=False)
    assert torch.equal(source, ref_source) and torch.equal(wall, ref_wall)
    ringed = S.reference(case, "index", 1)[0]
    assert (ringed != ref_wall).any()                        # with the score some tiles carry the ring
    with pytest.raises(ValueError, match="requires a score"):
        run(case, "score", 1, score=None)


def test_device_side_scores_and_frames_under_graph_replay(native):
    from aiko_services_amd.ops.reference import frame_wall_ref
    from aiko_services_amd.ops.wall import frame_wall, wall_shape
    case = S.CASES[0]
    h, w, tile = case
    kw = dict(rows=S.ROWS, cols=S.COLS, tile=tile, order="score", **S.options(case, 1), **S.COLOURS)
    frames, score = S.frames(h, w).cuda().clone(), S.scores().cuda()
    out = torch.empty(S.PAGES, *wall_shape(S.ROWS, S.COLS, tile, kw["gap"]), 3, dtype=torch.uint8, device="cuda")
    source = torch.empty(S.PAGES, S.N, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        frame_wall(frames, score, out=out, source=source, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frame_wall(frames, score, out=out, source=source, **kw)
    # the captured scene again, then one camera only (three tiles empty out), then all seven
    previous, emptied, filled = None, False, False
    for step, (seed, values) in enumerate([(0, S.SCORES), (1, [0, 9, 0, 0, 0, 0, 0]), (2, [1, 1, 1, 1, 1, 1, 2]),
                                           (3, S.SCORES)]):
        frames.copy_(S.frames(h, w, seed).cuda())
        score.copy_(S.scores(values).cuda())
        out.fill_(0x5A)
        source.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        eager_wall, eager_source = frame_wall(frames.clone(), score.clone(), pages=S.PAGES, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, eager_wall) and torch.equal(source, eager_source), step
        ref_wall, ref_source = frame_wall_ref(frames.cpu(), score.cpu(), pages=S.PAGES, **kw)
        assert torch.equal(source.cpu(), ref_source) and torch.equal(out.cpu(), ref_wall), step
        now = source.cpu().view(-1)
        if previous is not None:
            assert (now != previous).any()
            emptied = emptied or bool(((previous >= 0) & (now < 0)).any())
            filled = filled or bool(((previous < 0) & (now >= 0)).any())
        previous = now
    assert emptied and filled                                # tiles changed camera both ways


@pytest.mark.parametrize("width", [S.W, S.W16])
@pytest.mark.parametrize("order", ["index", "score"])
def test_guard_bands(native, width, order):
    """Index order shows camera 6 on the second page: its frame ends at the tensor's last byte,
    right in front of the guard."""
    from aiko_services_amd.ops.wall import frame_wall
    case = (S.H, width, (13, 37))
    frames, score = S.frames(S.H, width), S.scores()
    fresh_wall, fresh_source = run(case, order, 1)
    assert torch.equal(fresh_wall, S.reference(case, order, 1)[0])
    if order == "index":
        assert fresh_source[1, 0] == S.B - 1
    gf, cf = guarded(frames.shape, torch.uint8, "cuda", values=frames, name="frames")
    gs, cs = guarded(score.shape, torch.int32, "cuda", values=score, name="score")
    gw, cw = guarded(fresh_wall.shape, torch.uint8, "cuda", name="wall")
    gsrc, csrc = guarded(fresh_source.shape, torch.int32, "cuda", name="source")
    frame_wall(gf, gs, rows=S.ROWS, cols=S.COLS, tile=case[2], order=order, out=gw, source=gsrc,
               **S.options(case, 1), **S.COLOURS)
    torch.cuda.synchronize()
    for check in (cf, cs, cw, csrc):
        check()
    assert torch.equal(gf.cpu(), frames) and torch.equal(gs.cpu(), score)
    assert torch.equal(gw.cpu(), fresh_wall) and torch.equal(gsrc.cpu(), fresh_source)


def test_cameras_not_shown_may_hold_anything(native):
    case = S.CASES[0]
    base = run(case, "score", 1)
    frames = S.frames(case[0], case[1]).clone()
    g = torch.Generator().manual_seed(5)
    for cam in range(S.B):
        if cam not in S.SCORE_ORDER:
            frames[cam] = torch.randint(0, 256, frames[cam].shape, dtype=torch.uint8, generator=g)
    got = run(case, "score", 1, frames=frames)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    frames[S.SCORE_ORDER[-1]] ^= 0xFF                        # ... and a shown one does not
    assert (run(case, "score", 1, frames=frames)[0] != base[0]).any()


def test_refusals(native):
    from aiko_services_amd.ops.wall import frame_wall, wall_shape
    frames, score = S.frames().cuda(), S.scores().cuda()
    tile = (13, 37)
    shape = (S.PAGES, *wall_shape(S.ROWS, S.COLS, tile, 0), 3)
    black, red, white = 0, 255, 0xffffff

    def op(frames=frames, score=score, rows=S.ROWS, cols=S.COLS, tile=tile, gap=0, order=0, min_score=1, ring=0,
           label_scale=0, label_base=0, colours=(black, red, white, black), passes=3, wall=None, source=None, pages=S.PAGES):
        if wall is None:
            wall = torch.empty(pages, *wall_shape(rows, cols, tile, gap), 3, dtype=torch.uint8, device="cuda")
        if source is None:
            source = torch.empty(wall.shape[0], rows * cols, dtype=torch.int32, device="cuda")
        torch.ops.aiko.frame_wall_out(frames, score, rows, cols, tile[0], tile[1], gap, order, min_score, ring,
                                      label_scale, label_base, *colours, passes, wall, source)

    op()
    wide = torch.zeros(S.B, S.H, 2 * S.W, 3, dtype=torch.uint8, device="cuda")
    assert not wide[:, :, ::2].is_contiguous()
    for match, kw in [
            ("frames uint8", dict(frames=frames.float())),
            ("frames uint8", dict(frames=frames[..., :2].contiguous())),
            ("frames uint8", dict(frames=frames[0])),
            ("contiguous", dict(frames=wide[:, :, ::2])),
            ("GPU tensor", dict(frames=frames.cpu())),
            ("GPU tensor", dict(score=score.cpu())),
            ("GPU tensor", dict(wall=torch.empty(shape, dtype=torch.uint8))),
            ("GPU tensor", dict(source=torch.empty(S.PAGES, S.N, dtype=torch.int32))),
            ("score int32", dict(score=score.long())),
            ("score int32", dict(score=score[:-1])),
            ("score int32", dict(score=torch.zeros(S.B + 1, dtype=torch.int32, device="cuda"))),
            ("score int32", dict(score=torch.zeros(2 * S.B, dtype=torch.int32, device="cuda")[::2])),
            ("requires a score", dict(score=None, order=1)),
            ("never enlarges", dict(tile=(S.H + 1, 37), wall=torch.empty(shape, dtype=torch.uint8, device="cuda"))),
            ("never enlarges", dict(tile=(13, S.W + 1), wall=torch.empty(shape, dtype=torch.uint8, device="cuda"))),
            ("never enlarges", dict(tile=(0, 37), wall=torch.empty(shape, dtype=torch.uint8, device="cuda"))),
            ("1024 tiles", dict(rows=33, cols=32, tile=(1, 1), pages=1)),
            ("1024 tiles", dict(rows=0, cols=3, wall=torch.empty(shape, dtype=torch.uint8, device="cuda"))),
            ("gap", dict(gap=65)),
            ("gap", dict(gap=-1, wall=torch.empty(shape, dtype=torch.uint8, device="cuda"))),
            ("order 0", dict(order=2)),
            ("ring", dict(ring=7)),                          # 2 * 7 > 13
            ("ring", dict(ring=-1)),
            ("label_scale", dict(label_scale=5)),
            ("label_scale", dict(label_scale=-1)),
            ("label_base", dict(label_base=-1)),
            ("label_base", dict(label_base=2 ** 31 - 1)),
            ("colour components", dict(colours=(black, red, 0x1000000, black))),
            ("colour components", dict(colours=(-1, red, white, black))),
            ("passes", dict(passes=0)),
            ("passes", dict(passes=4)),
            ("wall uint8", dict(wall=torch.empty(S.PAGES, shape[1], shape[2] + 1, 3, dtype=torch.uint8, device="cuda"))),
            ("wall uint8", dict(wall=torch.empty(shape, dtype=torch.int8, device="cuda"))),
            ("wall uint8", dict(wall=torch.empty(S.PAGES, shape[1], 2 * shape[2], 3, dtype=torch.uint8,
                                                 device="cuda")[:, :, ::2])),
            ("source int32", dict(source=torch.empty(S.PAGES, S.N + 1, dtype=torch.int32, device="cuda"))),
            ("source int32", dict(source=torch.empty(S.PAGES, S.N, dtype=torch.int64, device="cuda"))),
            ("source int32", dict(source=torch.empty(S.PAGES * S.N, dtype=torch.int32, device="cuda")))]:
        with pytest.raises(RuntimeError, match=match):
            op(**kw)
    # frames of more than 2^23 pixels; more cameras than the selection ranks
    with pytest.raises(RuntimeError, match="exceeds 2\\^23"):
        op(frames=torch.zeros(1, 2049, 4096, 3, dtype=torch.uint8, device="cuda"), score=None, tile=(4, 4), pages=1)
    many = torch.zeros(4097, 1, 1, 3, dtype=torch.uint8, device="cuda")
    many_score = torch.zeros(4097, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="at most 4096"):
        op(frames=many, score=many_score, tile=(1, 1), order=1)
    op(frames=many, score=many_score, tile=(1, 1), order=0)                  # index order has no such limit
    # an output that overlaps an input
    big = torch.zeros(2 * max(frames.numel(), S.PAGES * shape[1] * shape[2] * 3), dtype=torch.uint8, device="cuda")
    inside = big[:frames.numel()].view(frames.shape)
    with pytest.raises(RuntimeError, match="wall and frames overlap"):
        op(frames=inside, wall=big[frames.numel() - 3:][:S.PAGES * shape[1] * shape[2] * 3].view(shape))
    op(frames=inside, wall=big[frames.numel():][:S.PAGES * shape[1] * shape[2] * 3].view(shape))   # adjacent: fine
    ints = torch.zeros(S.B + S.PAGES * S.N, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="source and score overlap"):
        op(score=ints[:S.B], source=ints[S.B - 1:S.B - 1 + S.PAGES * S.N].view(S.PAGES, S.N))
    # the front end's own checks
    for match, kw in [("order", dict(order="random")), ("larger than the frame", dict(tile=(51, 37))),
                      ("rows \\* cols", dict(rows=64, cols=17)), ("exceed", None), ("gap", dict(gap=65)),
                      ("ring", dict(ring=7)), ("label_scale", dict(label_scale=5)), ("label_base", dict(label_base=-1)),
                      ("alert", dict(alert=(0, 256, 0))), ("background", dict(background=(0, 0))),
                      ("label_fg", dict(label_fg=(0, 0, -1))), ("pages", dict(pages=0)), ("tile", dict(tile=(13,))),
                      ("integer", dict(gap=1.5))]:
        with pytest.raises(ValueError, match=match):
            if kw is None:
                frame_wall(torch.zeros(1, 2049, 4096, 3, dtype=torch.uint8, device="cuda"), rows=1, cols=1, tile=(4, 4))
            else:
                frame_wall(frames, score, **{**dict(rows=S.ROWS, cols=S.COLS, tile=tile), **kw})
    torch.cuda.synchronize()


# ---- the example pipeline -------------------------------------------------------------------

# SyntheticFrames slots are independent random pixels: at cell 16 two slots' cell means differ by a
# few luma levels, so threshold 1 makes the motion detector report moving cells from the second
# frame on (test_gpu_motion.py) and the wall ring its tiles
PIPE_B, PIPE_H, PIPE_W = 16, 96, 128
PIPE_FRAMES = 3
EXAMPLE = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/yolo/yolo_wall_gpu.json"


def _definition(lanes, sink=False):
    d = json.loads(EXAMPLE.read_text())
    assert d["graph"] == ["(SyntheticFrames (MotionDetector DetectionOverlay FrameWall (motion_cells: scores)) "
                          "JpegEncode JpegResults)"]
    d["parameters"]["gpu_lanes"] = lanes
    by_name = {e["name"]: e for e in d["elements"]}
    by_name["SyntheticFrames"]["parameters"].update(batch=PIPE_B, height=PIPE_H, width=PIPE_W, pool=4)
    by_name["MotionDetector"]["parameters"].update(threshold=1)
    wall = by_name["FrameWall"]["parameters"]
    assert (wall["rows"], wall["cols"], wall["order"]) == (4, 4, "index") and wall["ring"] > 0
    if sink:
        d["graph"] = ["(SyntheticFrames (MotionDetector DetectionOverlay FrameWall (motion_cells: scores)) "
                      "WallResults JpegEncode JpegResults)"]
        d["elements"].append({"name": "WallResults", "input": [{"name": "wall_sources", "type": "tensor"}],
                              "output": [{"name": "wall", "type": "result"}], "parameters": {},
                              "deploy": {"local": {"module": "aiko_services_amd.elements.gpu.wall"}}})
    return d


def _pipeline(lanes, sink=False):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<wall>", parse_pipeline_definition_dict(_definition(lanes, sink)),
                                     None, None, "c", [], 0, None, 60, queue_response=q)
    p.response_swag = True                     # the whole swag comes back, device tensors included
    return p, q


def _run_pipeline(lanes):
    p, q = _pipeline(lanes)
    # JpegEncode replaces ``images`` in the swag: keep what the element was given and what it gave
    element = p.pipeline_graph.get_node("FrameWall").element
    inner, seen = element.process_frame, []

    def spy(stream, images, scores=None):
        event, result = inner(stream, images, scores)
        assert scores is not None                            # the (motion_cells: scores) mapping
        seen.append({"frames": images.clone(), "scores": scores.clone(), "wall": result["images"].clone(),
                     "source": result["wall_sources"].clone()})
        return event, result

    element.process_frame = spy
    for i in range(PIPE_FRAMES):
        p.process_frame({"stream_id": "c", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        torch.cuda.synchronize()               # buffers are reused per lane: copy before the next frame
        # one JFIF file for the sixteen cameras
        assert swag["format"] == "jpeg" and len(swag["images"]) == 1 and bytes(swag["images"][0][:2]) == b"\xff\xd8"
    assert p.share["gpu_lanes"] == lanes and len(seen) == PIPE_FRAMES
    return seen, element


def test_wall_pipeline_matches_direct_calls(native):
    from aiko_services_amd.ops.reference import frame_wall_ref
    from aiko_services_amd.ops.wall import frame_wall
    one, element = _run_pipeline(1)
    params = json.loads(EXAMPLE.read_text())["elements"][3]["parameters"]
    kw = dict(rows=4, cols=4, tile=(PIPE_H // 4, PIPE_W // 4), gap=params["gap"], order="index",
              min_score=params["min_score"], ring=params["ring"], label_scale=params["label_scale"],
              label_base=params["label_base"], alert=tuple(json.loads(params["alert"])),
              background=tuple(json.loads(params["background"])))
    ringed = 0
    for i, o in enumerate(one):
        assert o["wall"].shape == (1, PIPE_H, PIPE_W, 3) and o["source"].view(-1).tolist() == list(range(16))
        wall, source = frame_wall(o["frames"], o["scores"], **kw)
        torch.cuda.synchronize()
        assert torch.equal(o["wall"], wall) and torch.equal(o["source"], source), i
        ref_wall, ref_source = frame_wall_ref(o["frames"], o["scores"], **kw)
        assert torch.equal(o["wall"].cpu(), ref_wall) and torch.equal(o["source"].cpu(), ref_source), i
        ringed += int((o["scores"] >= params["min_score"]).sum())
    print(f"wall pipeline: scores {[o['scores'].tolist() for o in one]}")
    assert ringed > 0 and int(one[0]["scores"].sum()) == 0   # warm-up frame: nothing moves, nothing ringed
    two, _ = _run_pipeline(2)
    for a, b in zip(one, two):
        for key in ("frames", "scores", "wall", "source"):
            assert torch.equal(a[key], b[key]), key


def test_wall_results_and_diagnostics(native):
    from aiko_services_amd.pipeline.stream import StreamEvent
    p, q = _pipeline(1, sink=True)
    for i in range(2):
        p.process_frame({"stream_id": "c", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        host = swag["wall"].wait()
        assert host["sources"].is_pinned() and host["sources"].device.type == "cpu"
        assert torch.equal(host["sources"], swag["wall_sources"].cpu())
        assert host["sources"].view(-1).tolist() == list(range(16))
    element = p.pipeline_graph.get_node("FrameWall").element
    good = torch.zeros(PIPE_B, PIPE_H, PIPE_W, 3, dtype=torch.uint8, device="cuda")
    event, out = element.process_frame(None, good)                             # scores are optional
    assert event == StreamEvent.OKAY and out["images"].shape == (1, PIPE_H, PIPE_W, 3)
    for args, text in (((good.float(),), "images uint8"), ((good[..., :2],), "images uint8"),
                       ((good.cpu(),), "images uint8"), ((None,), "images uint8"),
                       ((good, torch.zeros(PIPE_B, dtype=torch.int64, device="cuda")), "scores int32"),
                       ((good, torch.zeros(3, dtype=torch.int32, device="cuda")), "scores int32"),
                       ((good[:, :4, :4].contiguous(),), "ring")):              # a 1 x 1 tile cannot carry ring 3
        event, out = element.process_frame(None, *args)
        assert event == StreamEvent.ERROR and "FrameWall" in out["diagnostic"] and text in out["diagnostic"], out


def test_element_refuses_bad_parameters(native):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl

    def make(**params):                          # the element alone behind a frame source
        d = _definition(1)
        d["graph"] = ["(SyntheticFrames FrameWall)"]
        d["elements"] = [e for e in d["elements"] if e["name"] in ("SyntheticFrames", "FrameWall")]
        wall = {e["name"]: e for e in d["elements"]}["FrameWall"]
        wall["input"] = wall["input"][:1]
        wall["parameters"].update(params)
        p = PipelineImpl.create_pipeline("<wall>", parse_pipeline_definition_dict(d), None, None, "c", [], 0, None,
                                         60, queue_response=queue.Queue())
        return p.pipeline_graph.get_node("FrameWall").element

    for params in (dict(rows=0), dict(rows=33, cols=32), dict(gap=65), dict(order="random"), dict(label_scale=5),
                   dict(alert="[0, 0, 256]"), dict(background="[0, 0]"), dict(pages=0), dict(tile_height=10)):
        with pytest.raises(ValueError, match="FrameWall"):
            make(**params)
    element = make(tile_height=10, tile_width=20, order="score")
    from aiko_services_amd.pipeline.stream import StreamEvent
    good = torch.zeros(PIPE_B, PIPE_H, PIPE_W, 3, dtype=torch.uint8, device="cuda")
    event, out = element.process_frame(None, good)
    assert event == StreamEvent.ERROR and "requires scores" in out["diagnostic"]
    event, out = element.process_frame(None, good, torch.ones(PIPE_B, dtype=torch.int32, device="cuda"))
    assert event == StreamEvent.OKAY and out["images"].shape == (1, 40, 80, 3)
