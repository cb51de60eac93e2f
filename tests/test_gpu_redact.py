"""Detection redaction on the MI355X (``redact_ops.hip``): bit for bit against
``redact_detections_ref`` on the shared scene (redact_scenes.py), in place, the device-side count
under hipGraph replay, guard bands, refusals, more rows than one culling round, tiles inside a box,
and the DetectionRedact element in its example pipeline against the same kernel called directly."""
import json
import queue
from pathlib import Path

import numpy as np
import pytest
import torch

import redact_scenes as S
from kernel_guard import guarded

pytestmark = pytest.mark.gpu

FILL_T = torch.tensor(S.FILL, dtype=torch.uint8)


def run(frames, det, count, k=S.K, out=None, **kw):
    from aiko_services_amd.ops.redact import redact_detections
    dev = lambda x: None if x is None else x.cuda()  # noqa: E731
    kw["select"], kw["labels"] = dev(kw.get("select")), dev(kw.get("labels"))
    res = redact_detections(frames.cuda(), det.cuda(), count.cuda(), k, out=out, **kw)
    torch.cuda.synchronize()
    return res.cpu()


def _slots(with_select, with_labels, k=S.K):
    return dict(select=S.scene()["select"] if with_select else None, labels=S.labels(k) if with_labels else None)


@pytest.mark.parametrize("width", [S.W, S.W4])
@pytest.mark.parametrize("block", [4, 16, 32])
def test_equals_reference(native, width, block):
    frames, det, count = S.inputs(width)
    before = frames.clone()
    for mode in ("pixelate", "fill"):
        for with_select in (False, True):
            for with_labels in (False, True):
                got = run(frames, det, count, mode=mode, block=block, fill=S.FILL, **_slots(with_select, with_labels))
                ref = S.reference(width, block, mode, with_select, with_labels)
                diff = (got != ref).any(-1)
                print(f"redact W={width} block={block} {mode} select={with_select} labels={with_labels}: "
                      f"{int(diff.sum())} of {diff.numel()} pixels differ {torch.nonzero(diff)[:5].tolist()}")
                assert torch.equal(got, ref)
                assert (ref != frames).any()
    assert torch.equal(frames, before)


def test_block_8_and_defaults(native):
    frames, det, count = S.inputs()
    assert torch.equal(run(frames, det, count, block=8), S.reference(S.W, 8))
    assert torch.equal(run(frames, det, count), S.reference(S.W, 16))             # pixelate, block 16, every class
    black = frames.clone()
    black[S.coverage()] = 0
    assert torch.equal(run(frames, det, count, mode="fill"), black)               # fill defaults to black


def test_margin_covers_the_rects_of_roi_crop(native):
    from aiko_services_amd.ops.roi import roi_crop
    frames, det, count = S.inputs()
    got = run(frames, det, count, mode="fill", block=4, fill=S.FILL, margin=0.15)
    assert torch.equal(got, S.reference(S.W, 4, "fill", margin=0.15))
    _, rois = roi_crop(frames.cuda(), det.cuda(), count.cuda(), S.K, (8, 8), 0.15)
    rois = rois.cpu().view(S.B, S.K, 4).tolist()
    assert rois[1][0] == [54, 27, 107, 56]
    mask = torch.zeros(S.B, S.H, S.W, dtype=torch.bool)
    for b in range(S.B):
        for x0, y0, x1, y1 in rois[b]:
            mask[b, y0:y1, x0:x1] = True
    assert torch.equal((got == FILL_T).all(-1), mask)                           # the covered region, read off the picture
    assert torch.equal(got[~mask], frames[~mask])
    assert torch.equal(run(frames, det, count, block=16, margin=0.15), S.reference(S.W, 16, margin=0.15))


@pytest.mark.parametrize("width", [S.W, S.W4])
def test_in_place_equals_out_of_place(native, width):
    from aiko_services_amd.ops.redact import redact_detections
    frames, det, count = S.inputs(width)
    sel, lab = S.scene()["select"].cuda(), S.labels().cuda()
    for block in (4, 32):
        for mode in ("pixelate", "fill"):
            for with_select in (False, True):
                buf = frames.cuda().clone()
                res = redact_detections(buf, det.cuda(), count.cuda(), S.K, mode=mode, block=block, fill=S.FILL,
                                        select=sel if with_select else None, labels=lab if with_select else None,
                                        out=buf)
                torch.cuda.synchronize()
                assert res is buf
                assert torch.equal(buf.cpu(), S.reference(width, block, mode, with_select, with_select)), \
                    (block, mode, with_select)


def test_unused_rows_and_slots_are_never_read(native):
    frames, det, count = S.inputs()
    k = 4                                                    # frame 1: count 5 > k
    sel, labels = S.scene()["select"], S.labels(k)
    base = run(frames, det, count, k, block=8, select=sel, labels=labels)
    assert torch.equal(base, S.reference(S.W, 8, "pixelate", True, True, k=k))
    g = torch.Generator().manual_seed(3)
    for fill in ("nan", "garbage"):
        d, lab = det.clone(), labels.clone().view(S.B, k)
        for b, c in enumerate(S.COUNTS):
            n = S.MAX_DET - c
            d[b, c:] = S.NAN if fill == "nan" else (torch.rand(n, 6, generator=g) - 0.5) * 1e4
            u = min(c, k)
            lab[b, u:] = -2 ** 31 if fill == "nan" else torch.randint(-10 ** 9, 10 ** 9, (k - u,), generator=g).int()
        d[1, 2] = det[1, 2]                                  # the NaN row below the count stays as it is
        d[1, 2, 4:] = S.NAN if fill == "nan" else 1e9       # ... but its score and class are never used
        lab[1, 2] = 10 ** 9
        got = run(frames, d, count, k, block=8, select=sel, labels=lab.reshape(-1))
        assert torch.equal(got, base), fill
    # rows at and past k are unused too, whatever the count says
    d = det.clone()
    d[:, k:] = S.NAN
    assert torch.equal(run(frames, d, count, k, block=8, select=sel, labels=labels), base)
    # without a table no class is looked at: poison in every label changes nothing
    poison = torch.full((S.B * k,), -2 ** 31, dtype=torch.int32)
    assert torch.equal(run(frames, det, count, k, block=8, labels=poison), S.reference(S.W, 8, k=k))


def test_device_side_count_under_graph_replay(native):
    from aiko_services_amd.ops.redact import redact_detections
    from aiko_services_amd.ops.reference import roi_rects_ref
    frames, det, count = (x.cuda() for x in S.inputs())
    sel, labels = S.scene()["select"].cuda(), S.labels().cuda()
    out = torch.empty_like(frames)
    kw = dict(mode="pixelate", block=8, select=sel)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        redact_detections(frames, det, count, S.K, labels=labels, out=out, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        redact_detections(frames, det, count, S.K, labels=labels, out=out, **kw)
    first = None
    # the captured scene again, then two rewrites: frame 0 gets boxes, frame 1 loses them, frame 2
    # changes its boxes; then the reverse
    for step, (seed, counts, order) in enumerate([(0, S.COUNTS, [0, 1, 2]), (5, [2, 0, 5], [1, 2, 0]),
                                                  (6, [1, 3, 0], [2, 0, 1])]):
        frames.copy_(S.frames(seed).cuda())
        det.copy_(S.det([S.BOXES[i] for i in order]).cuda())
        count.copy_(torch.tensor(counts, dtype=torch.int32).cuda())
        labels.copy_(S.labels(S.K, seed).cuda())
        out.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        eager = redact_detections(frames.clone(), det.clone(), count.clone(), S.K, labels=labels.clone(), **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, eager), step
        assert (out != frames).any()
        rois = roi_rects_ref(det.cpu(), count.cpu(), S.K, (S.H, S.W), 0.0)
        valid = rois[:, 2] > rois[:, 0]
        if first is None:
            first = valid
            assert torch.equal(out.cpu(), S.reference(S.W, 8, "pixelate", True, True))
        else:
            assert (valid & ~first).any() and (~valid & first).any()     # slots flipped both ways


@pytest.mark.parametrize("width", [S.W, S.W4])
@pytest.mark.parametrize("mode", ["pixelate", "fill"])
def test_guard_bands(native, width, mode):
    from aiko_services_amd.ops.redact import redact_detections
    frames, det, count = S.inputs(width)
    sel, labels = S.scene()["select"], S.labels()
    block = 16
    fresh = run(frames, det, count, mode=mode, block=block, fill=S.FILL, select=sel, labels=labels)
    assert torch.equal(fresh, S.reference(width, block, mode, True, True))
    ops = {"frames": (frames, torch.uint8), "det": (det, torch.float32), "count": (count, torch.int32),
           "labels": (labels, torch.int32), "select": (sel, torch.uint8)}
    g, checks = {}, []
    for name, (value, dtype) in ops.items():
        g[name], check = guarded(value.shape, dtype, "cuda", values=value, name=name)
        checks.append(check)
    go, co = guarded(frames.shape, torch.uint8, "cuda", name="out")
    kw = dict(mode=mode, block=block, fill=S.FILL, select=g["select"], labels=g["labels"])
    redact_detections(g["frames"], g["det"], g["count"], S.K, out=go, **kw)
    torch.cuda.synchronize()
    for check in checks + [co]:
        check()
    for name, (value, _) in ops.items():                                 # no input changed (bytes: NaNs inside)
        assert torch.equal(g[name].cpu().view(torch.uint8), value.contiguous().view(torch.uint8)), name
    assert torch.equal(go.cpu(), fresh)
    # the corner box of the last frame (slot label 3: selected) ends at the tensor's last byte, right
    # in front of the 0xA5 guard: redacted up to it
    corner = go[-1, 50:, 100:].cpu()
    if mode == "fill":
        assert (corner == FILL_T).all()
    else:
        y0, x0 = S.H // block * block, width // block * block            # the last, partial cell
        cell = frames[-1, y0:, x0:].numpy().astype(np.int64)
        mean = np.floor(cell.sum((0, 1)) / (cell.shape[0] * cell.shape[1]) + 0.5)
        assert (go[-1, y0:, x0:].cpu().numpy() == mean).all()
    # the same, redacted in place between the guards
    redact_detections(g["frames"], g["det"], g["count"], S.K, out=g["frames"], **kw)
    torch.cuda.synchronize()
    for check in checks:
        check()
    assert torch.equal(g["frames"].cpu(), fresh)


def test_refusals(native):
    from aiko_services_amd.ops.redact import redact_detections
    frames, det, count = (x.cuda() for x in S.inputs())
    sel, labels = S.scene()["select"].cuda(), S.labels().cuda()
    B, H, W, K = S.B, S.H, S.W, S.K

    def call(frames=frames, det=det, count=count, k=K, **kw):
        return redact_detections(frames, det, count, k, **kw)

    wide = torch.zeros(B, H, 2 * W, 3, dtype=torch.uint8, device="cuda")
    assert not wide[:, :, ::2].is_contiguous()
    for match, kw in [
            ("frames uint8", dict(frames=frames.float())),
            ("frames uint8", dict(frames=frames[..., :2].contiguous())),
            ("contiguous", dict(frames=wide[:, :, ::2])),
            ("det fp32", dict(det=det.double())),
            ("det fp32", dict(det=det[:, :, :5].contiguous())),
            ("det fp32", dict(det=det[:2])),
            ("contiguous", dict(det=det.transpose(0, 1).contiguous().transpose(0, 1))),
            ("count int32", dict(count=count.long())),
            ("count int32", dict(count=count[:2])),
            ("k <= max_det", dict(k=S.MAX_DET + 1)),
            ("k <= max_det", dict(k=0)),
            ("labels int32", dict(labels=labels.long())),
            ("labels int32", dict(labels=labels[:-1])),
            ("labels int32", dict(labels=labels.view(B, K))),
            ("select uint8", dict(select=sel.int())),
            ("select uint8", dict(select=sel[:0])),
            ("select uint8", dict(select=sel.view(1, -1))),
            ("select uint8", dict(select=torch.zeros(2 * S.SELECT_N, dtype=torch.uint8, device="cuda")[::2])),
            ("block in", dict(block=12)),
            ("block in", dict(block=2)),
            ("block in", dict(block=64)),
            ("block in", dict(block=0, mode="fill")),
            ("fill components", dict(fill=(0, 256, 0))),
            ("fill components", dict(fill=(-1, 0, 0), mode="fill")),
            ("margin", dict(margin=-0.1)),
            ("margin", dict(margin=float("inf"))),
            ("margin", dict(margin=S.NAN)),
            ("out uint8", dict(out=torch.empty(B, H, W + 1, 3, dtype=torch.uint8, device="cuda"))),
            ("out uint8", dict(out=torch.empty(B, H, W, 3, dtype=torch.int8, device="cuda"))),
            ("contiguous", dict(out=wide[:, :, ::2])),
            ("GPU tensor", dict(frames=frames.cpu())),
            ("GPU tensor", dict(det=det.cpu())),
            ("GPU tensor", dict(count=count.cpu())),
            ("GPU tensor", dict(labels=labels.cpu())),
            ("GPU tensor", dict(select=sel.cpu())),
            ("GPU tensor", dict(out=torch.empty(B, H, W, 3, dtype=torch.uint8)))]:
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    with pytest.raises(RuntimeError, match="mode 0"):                         # the operator's own check
        torch.ops.aiko.redact_detections_out(frames, det, count, K, None, None, 2, 16, 0, 0.0, torch.empty_like(frames))
    with pytest.raises(ValueError, match="mode"):                             # the front end's
        call(mode="blur")
    with pytest.raises(ValueError, match="fill"):
        call(fill=(0, 0))
    # partial overlap: out starts one frame into the storage of frames
    big = torch.zeros(B + 1, H, W, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="overlaps"):
        call(frames=big[:B], out=big[1:])
    call(frames=big[:2], det=det[:2], count=count[:2], out=big[2:])           # adjacent, disjoint: fine
    with pytest.raises(RuntimeError, match="grid limit"):
        call(frames=torch.zeros(65536, 1, 1, 3, dtype=torch.uint8, device="cuda"),
             det=torch.zeros(65536, 1, 6, device="cuda"),
             count=torch.zeros(65536, dtype=torch.int32, device="cuda"), k=1)
    torch.cuda.synchronize()


def many_rows_scene():
    """300 small boxes from a seed in one 96 x 260 frame, classes 0..8, the even ones selected."""
    from aiko_services_amd.ops.redact import class_select
    n, h, w = 300, 96, 260
    g = torch.Generator().manual_seed(11)
    frames = torch.randint(0, 256, (1, h, w, 3), dtype=torch.uint8, generator=g)
    bw, bh = 3 + torch.rand(n, generator=g) * 9, 3 + torch.rand(n, generator=g) * 9
    x1, y1 = torch.rand(n, generator=g) * (w - bw), torch.rand(n, generator=g) * (h - bh)
    det = torch.stack([x1, y1, x1 + bw, y1 + bh, torch.rand(n, generator=g),
                       torch.randint(0, 9, (n,), generator=g).float()], -1)[None].contiguous()
    return frames, det, class_select([0, 2, 4, 6, 8], 9)


def test_more_rows_than_one_culling_round(native):
    """300 rows per frame (the YOLO bench's max_det) take two culling rounds: the covered mask of
    the first round is kept and the second round's rows are added to it."""
    from aiko_services_amd.ops.reference import redact_detections_ref
    frames, det, sel = many_rows_scene()
    n = det.shape[1]
    assert n > S.CHUNK
    count = torch.tensor([n], dtype=torch.int32)
    for select in (None, sel):
        ref = redact_detections_ref(frames, det, count, n, block=8, select=select)
        late = redact_detections_ref(frames, det, torch.tensor([S.CHUNK], dtype=torch.int32), n, block=8, select=select)
        assert (ref != late).any()                           # rows of the second round are visible
        assert torch.equal(run(frames, det, count, n, block=8, select=select), ref)
    assert torch.equal(run(frames, det, count, n, mode="fill", fill=S.FILL),
                       redact_detections_ref(frames, det, count, n, mode="fill", fill=S.FILL))


@pytest.mark.parametrize("width", [S.W, S.W4])
def test_whole_frame_box(native, width):
    """Every tile lies inside the rect (no walk over the list); frame 1 carries the same box under a
    deselected class and stays as it is."""
    from aiko_services_amd.ops.redact import class_select
    from aiko_services_amd.ops.reference import redact_detections_ref
    frames = S.frames(9, width)[:2].contiguous()
    det = torch.zeros(2, 3, 6)
    det[:, 0] = torch.tensor([-5.0, -5.0, width + 5.0, S.H + 5.0, 0.9, 0.0])
    det[:, 1] = torch.tensor([20.0, 10.0, 50.0, 40.0, 0.8, 0.0])               # a second row inside the first
    det[1, :, 5] = 1.0
    count = torch.tensor([2, 2], dtype=torch.int32)
    sel = class_select([0], 2)
    for block in S.BLOCKS:
        got = run(frames, det, count, 3, block=block, select=sel)
        assert torch.equal(got, redact_detections_ref(frames, det, count, 3, block=block, select=sel)), block
        assert torch.equal(got[1], frames[1])
        for y0 in range(0, S.H, block):                        # every cell flat
            for x0 in range(0, width, block):
                cell = got[0, y0:y0 + block, x0:x0 + block]
                assert (cell == cell[0, 0]).all(), (block, y0, x0)
    buf = frames.cuda().clone()
    run(buf, det, count, 3, out=buf, mode="fill", fill=S.FILL, select=sel)
    assert (buf[0].cpu() == FILL_T).all() and torch.equal(buf[1].cpu(), frames[1])


# ---- the example pipeline -------------------------------------------------------------------

# conf 0.2987 on 240 x 320 noise frames keeps 1-3 boxes per frame of the seeded YOLOv8-n, so with 4
# slots some are used and some are empty (the threshold's derivation: test_gpu_roi.py)
PIPE_CONF = 0.2987
PIPE_K = 4
EXAMPLES = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/yolo"


def _definition(lanes):
    d = json.loads((EXAMPLES / "yolo_redact_gpu.json").read_text())
    assert d["graph"] == ["(SyntheticFrames YoloDetector DetectionRedact DetectionOverlay RgbToYuv)"]
    d["parameters"]["gpu_lanes"] = lanes
    by_name = {e["name"]: e for e in d["elements"]}
    by_name["SyntheticFrames"]["parameters"].update(batch=2, height=240, width=320)
    by_name["YoloDetector"]["parameters"].update(autotune=False, graph=True, conf=PIPE_CONF)
    assert by_name["DetectionRedact"]["parameters"]["classes"] == "[0]"
    by_name["DetectionRedact"]["parameters"].update(rois=PIPE_K)
    del by_name["DetectionRedact"]["parameters"]["classes"]         # every class
    by_name["DetectionOverlay"]["parameters"].update(rois=PIPE_K)
    return d


def _run_pipeline(lanes, frames=3):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<redact>", parse_pipeline_definition_dict(_definition(lanes)),
                                     None, None, "c", [], 0, None, 60, queue_response=q)
    p.response_swag = True                     # the whole swag comes back, device tensors included
    # later elements replace ``images`` in the swag: keep what the element was given and what it gave
    element = p.pipeline_graph.get_node("DetectionRedact").element
    inner, seen = element.process_frame, []

    def spy(stream, images, *args, **kw):
        source = images.clone()
        event, result = inner(stream, images, *args, **kw)
        assert result["images"].data_ptr() != images.data_ptr()
        seen.append((source, result["images"].clone()))
        return event, result

    element.process_frame = spy
    outs = []
    for i in range(frames):
        p.process_frame({"stream_id": "c", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        torch.cuda.synchronize()               # buffers are reused per lane: copy before the next frame
        outs.append({"source": seen[i][0], "redacted": seen[i][1], "nv12": swag["images"].clone(),
                     "det": swag["detections"].clone(), "count": swag["counts"].clone()})
    assert p.share["gpu_lanes"] == lanes and len(seen) == frames
    return outs


def test_redact_pipeline_matches_direct_calls(native):
    from aiko_services_amd.ops.redact import redact_detections
    from aiko_services_amd.ops.reference import redact_detections_ref, roi_rects_ref
    one = _run_pipeline(1)
    redacted = unused = 0
    for o in one:
        det, count = o["det"], o["count"]
        assert o["nv12"].shape != o["source"].shape                            # NV12 left the pipeline
        direct = redact_detections(o["source"], det, count, PIPE_K)
        torch.cuda.synchronize()
        assert torch.equal(o["redacted"], direct)
        assert torch.equal(o["redacted"].cpu(), redact_detections_ref(o["source"], det, count, PIPE_K))
        rois = roi_rects_ref(det.cpu(), count.cpu(), PIPE_K, o["source"].shape[1:3], 0.0)
        valid = rois[:, 2] > rois[:, 0]
        redacted += int(valid.sum())
        unused += int((~valid).sum())
        for b in range(2):                                   # a frame changes iff it has a used row
            assert bool((o["redacted"][b] != o["source"][b]).any()) == bool(valid[b * PIPE_K:(b + 1) * PIPE_K].any())
    print(f"redact pipeline: conf {PIPE_CONF}: {redacted} boxes redacted, {unused} slots unused")
    assert redacted >= 1 and unused >= 1
    two = _run_pipeline(2)
    for a, b in zip(one, two):
        for key in ("source", "redacted", "nv12", "det", "count"):
            assert torch.equal(a[key], b[key]), key


def test_element_refuses_bad_parameters_and_shapes(native):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    from aiko_services_amd.pipeline.stream import StreamEvent

    def make(**params):                          # the element alone behind a frame source: no detector to build
        d = _definition(1)
        d["graph"] = ["(SyntheticFrames DetectionRedact)"]
        d["elements"] = [e for e in d["elements"] if e["name"] in ("SyntheticFrames", "DetectionRedact")]
        {e["name"]: e for e in d["elements"]}["DetectionRedact"]["parameters"].update(params)
        p = PipelineImpl.create_pipeline("<redact>", parse_pipeline_definition_dict(d), None, None, "c", [], 0, None,
                                         60, queue_response=queue.Queue())
        return p.pipeline_graph.get_node("DetectionRedact").element

    for params in (dict(block=12), dict(mode="blur"), dict(fill="[0, 0, 256]"), dict(fill="[0, 0]"), dict(margin=-1.0),
                   dict(rois=0), dict(classes="[-1]")):
        with pytest.raises(ValueError, match="DetectionRedact|class_select"):
            make(**params)
    element = make(classes="[0, 90]")
    assert element._select_host.shape == (91,)                                 # class_count grows to max + 1
    frames, det, count = (x.cuda() for x in S.inputs())
    for args in ((frames.float(), det, count), (frames, det[:2], count), (frames, det[:, :2], count),
                 (frames, det, count.long()), (frames, det, count, torch.zeros(3, dtype=torch.int32, device="cuda"))):
        event, result = element.process_frame(None, *args)
        assert event == StreamEvent.ERROR and "DetectionRedact" in result["diagnostic"]
