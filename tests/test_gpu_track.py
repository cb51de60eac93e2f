"""The tracker kernel (``ops.track.track_detections``, track_ops.hip) against the CPU reference, bit
for bit and step by step, on the scenes of track_scenes.py; then the elements in the example
pipeline against direct calls."""
import json
import queue
from pathlib import Path

import pytest
import torch

import track_scenes as S
from kernel_guard import guarded
from track_scenes import B, K, MAX_DET, T

pytestmark = pytest.mark.gpu

NAMES = ("ids", "hits", "labels", "boxes", "meta", "issued")
SCENES = {**S.SCRIPTED, "walk": S.WALK, "walk_64x64": S.WALK_FULL, "walk_1x1": S.WALK_ONE}


def _flat(step):
    ids, hits, labels, state = step
    return [t.cpu() for t in (ids, hits, labels, *state)]


def _assert_step(got, want, where):
    for name, g, w in zip(NAMES, _flat(got), _flat(want)):
        assert g.dtype == w.dtype and torch.equal(g, w), f"{where}: {name}\n{g}\n{w}"


def _run(scene, frames=None):
    """Every step of ``scene`` on the device from the empty state: [(ids, hits, labels, state), ...]."""
    from aiko_services_amd.ops.track import new_state, track_detections
    state = new_state(scene.batch, scene.tracks, "cuda")
    steps = []
    for det, count in (scene.frames if frames is None else frames):
        ids, hits, labels, state = track_detections(det.cuda(), count.cuda(), state, scene.k, **scene.kw)
        steps.append((ids, hits, labels, state))
    torch.cuda.synchronize()
    return steps


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_step_equals_reference(native, name):
    scene = SCENES[name]
    want = S.reference(scene)
    got = _run(scene)
    for i, (g, w) in enumerate(zip(got, want)):
        _assert_step(g, w, f"{name}, frame {i}")
    if name == "walk_64x64":                                # every lane owns a live track
        assert all(bool((g[3].meta[:, :, 0] != 0).all()) for g in got[1:])


def test_rows_past_count_are_never_read(native):
    scene = S.WALK
    base = _run(scene)
    g = torch.Generator().manual_seed(3)
    for fill in ("nan", "garbage"):
        frames = []
        for det, count in scene.frames:
            d = det.clone()
            for b in range(scene.batch):
                n = min(max(int(count[b]), 0), scene.k)     # rows k .. count are not read either
                rest = d.shape[1] - n
                d[b, n:] = S.NAN if fill == "nan" else (torch.rand(rest, 6, generator=g) - 0.5) * 1e4
            frames.append((d, count))
        for i, (got, want) in enumerate(zip(_run(scene, frames), base)):
            _assert_step(got, want, f"{fill}, frame {i}")


def test_device_side_state_under_graph_replay(native):
    from aiko_services_amd.ops.track import TrackState, new_state, track_detections
    scene = S.WALK
    eager = _run(scene)
    det, count = (t.cuda() for t in scene.frames[0])
    state, state_out = new_state(scene.batch, scene.tracks, "cuda"), new_state(scene.batch, scene.tracks, "cuda")
    outs = [torch.empty(scene.batch * scene.k, dtype=torch.int32, device="cuda") for _ in range(3)]

    def step():
        track_detections(det, count, state, scene.k, state_out=state_out, ids=outs[0], hits=outs[1],
                         labels=outs[2], **scene.kw)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in state:
        t.zero_()
    for i, (d, c) in enumerate(scene.frames):
        det.copy_(d)
        count.copy_(c)
        for t in (*outs, *state_out):                       # poison: every element must be rewritten
            t.view(torch.uint8).fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        _assert_step((*outs, state_out), eager[i], f"replay {i}")
        for dst, src in zip(state, state_out):
            dst.copy_(src)
    assert isinstance(eager[0][3], TrackState)


def test_guard_bands(native):
    from aiko_services_amd.ops.track import TrackState, track_detections
    scene = S.WALK
    fresh = _run(scene)
    n, t, k = scene.batch, scene.tracks, scene.k
    at = 5                                                  # a frame in mid-scene: a populated table
    det, count = scene.frames[at]
    before = fresh[at - 1][3]
    checks = []

    def g(shape, dtype, values=None, name=""):
        view, check = guarded(shape, dtype, "cuda", values=values, name=name)
        checks.append(check)
        return view

    gd = g(det.shape, torch.float32, det, "det")
    gc = g(count.shape, torch.int32, count, "count")
    gin = TrackState(g((n, t, 4), torch.float32, before.boxes, "boxes"), g((n, t, 4), torch.int32, before.meta, "meta"),
                     g((n,), torch.int32, before.issued, "issued"))
    gout = TrackState(g((n, t, 4), torch.float32, name="boxes_out"), g((n, t, 4), torch.int32, name="meta_out"),
                      g((n,), torch.int32, name="issued_out"))
    outs = [g((n * k,), torch.int32, name=name) for name in ("ids", "hits", "labels")]
    track_detections(gd, gc, gin, k, state_out=gout, ids=outs[0], hits=outs[1], labels=outs[2], **scene.kw)
    torch.cuda.synchronize()
    for check in checks:
        check()
    _assert_step((*outs, gout), fresh[at], "guarded")
    # no element of any output kept its poison (int32 0xA5A5A5A5, the fp32 NaN)
    for x in (*outs, gout.meta, gout.issued):
        assert not (x.view(torch.uint8).view(-1, 4) == 0xA5).all(1).any()
    assert torch.isfinite(gout.boxes).all()
    # the inputs are only read
    assert torch.equal(gin.boxes, before.boxes) and torch.equal(gin.meta, before.meta)


def test_refusals(native):
    from aiko_services_amd.ops.track import TrackState, new_state, track_detections
    det, count = (t.cuda() for t in S.SCRIPTED["greedy"].frames[0])
    state = new_state(B, T, "cuda")

    def refuse(match, det=det, count=count, state=state, k=K, **kw):
        with pytest.raises(RuntimeError, match=match):
            track_detections(det, count, state, k, **kw)

    refuse("det fp32", det=det.double())
    refuse("count int32", count=count.long())
    refuse("state boxes fp32", state=TrackState(state.boxes, state.meta.float(), state.issued))
    refuse("state boxes fp32", state=TrackState(state.boxes, state.meta, state.issued.long()))
    refuse("boxes fp32", state=TrackState(state.boxes.double(), state.meta, state.issued))
    refuse("state_out boxes fp32", state_out=TrackState(state.boxes.clone(), state.meta.clone().long(),
                                                        state.issued.clone()))
    refuse("ids, hits and labels int32", ids=torch.empty(B * K, dtype=torch.int64, device="cuda"))
    refuse("ids, hits and labels int32", labels=torch.empty(B * K + 1, dtype=torch.int32, device="cuda"))
    wide = torch.zeros(B, MAX_DET, 12, device="cuda")
    assert not wide[:, :, ::2].is_contiguous()
    refuse("contiguous", det=wide[:, :, ::2])
    refuse("contiguous", state=TrackState(torch.zeros(B, T, 8, device="cuda")[:, :, ::2], state.meta, state.issued))
    refuse("GPU tensor", det=det.cpu())
    refuse("GPU tensor", state_out=new_state(B, T, "cpu"))
    if torch.cuda.device_count() > 1:
        refuse("device", count=count.to("cuda:1"))
    refuse("1 <= k <= 64", k=0)
    refuse("1 <= k <= 64", k=65, det=torch.zeros(B, 80, 6, device="cuda"))
    refuse("k <= max_det", k=MAX_DET + 1)
    refuse("track slots", state=new_state(B, 65, "cuda"))
    refuse("track slots", state=new_state(B, 0, "cuda"))
    refuse("state of", state=new_state(B + 1, T, "cuda"))
    refuse("state_out boxes fp32", state_out=new_state(B, T + 1, "cuda"))
    big = 65536
    refuse("grid limit", det=torch.zeros(big, 1, 6, device="cuda"), k=1, state=new_state(big, 1, "cuda"),
           count=torch.zeros(big, dtype=torch.int32, device="cuda"))
    for iou in (0.0, -0.3, 1.5, float("nan")):
        refuse("0 < iou <= 1", iou=iou)
    refuse("max_age >= 0", max_age=-1)
    refuse("label_mod >= 1", label_mod=0)
    # an output over an input, and over another output
    refuse("boxes_out and boxes overlap", state_out=state)
    refuse("meta_out and meta overlap", state_out=TrackState(state.boxes.clone(), state.meta, state.issued.clone()))
    shared = torch.zeros(B * K, dtype=torch.int32, device="cuda")
    refuse("labels and count overlap", count=shared[:B], labels=shared)
    refuse("hits and ids overlap", ids=shared, hits=shared)
    both = torch.zeros(2 * B, dtype=torch.int32, device="cuda")
    refuse("issued_out and issued overlap", state=TrackState(state.boxes, state.meta, both[:B]),
           state_out=TrackState(state.boxes.clone(), state.meta.clone(), both[B - 1:2 * B - 1]))
    # iou = 1 and max_age = 0 are inside the bounds
    track_detections(det, count, state, K, iou=1.0, max_age=0, label_mod=1)
    torch.cuda.synchronize()


# ---- the example pipeline -------------------------------------------------------------------

# conf 0.2987 on 240 x 320 noise frames keeps 1-3 boxes per frame of the seeded YOLOv8-n, so with 4
# slots some are used and some are empty (the threshold's derivation: test_gpu_roi.py).  The frame
# pool rotates 4 batches: frames 4 and 5 show frames 0 and 1 again, whose tracks (max_age 4) are
# still alive and are matched again.
PIPE_CONF = 0.2987
PIPE_K = 4
PIPE_TRACKS = 32
PIPE_MAX_AGE = 4
PIPE_FRAMES = 6
EXAMPLE = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/yolo/yolo_track_gpu.json"


def _definition(lanes, sink=False):
    d = json.loads(EXAMPLE.read_text())
    d["parameters"]["gpu_lanes"] = lanes
    by_name = {e["name"]: e for e in d["elements"]}
    by_name["SyntheticFrames"]["parameters"].update(batch=2, height=240, width=320, pool=4)
    by_name["YoloDetector"]["parameters"].update(autotune=False, graph=True, conf=PIPE_CONF)
    by_name["DetectionTracker"]["parameters"].update(rois=PIPE_K, tracks=PIPE_TRACKS, max_age=PIPE_MAX_AGE)
    by_name["DetectionOverlay"]["parameters"].update(rois=PIPE_K)
    if sink:
        d["graph"] = ["(SyntheticFrames YoloDetector DetectionTracker DetectionOverlay TrackResults)"]
        tensor = lambda name: {"name": name, "type": "tensor"}  # noqa: E731
        d["elements"].append({"name": "TrackResults",
                              "input": [tensor("detections"), tensor("counts"), tensor("track_ids"),
                                        tensor("track_hits")],
                              "output": [{"name": "tracks", "type": "result"}], "parameters": {},
                              "deploy": {"local": {"module": "aiko_services_amd.elements.gpu.track"}}})
    return d


def _pipeline(lanes, sink=False):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<track>", parse_pipeline_definition_dict(_definition(lanes, sink)),
                                     None, None, "c", [], 0, None, 60, queue_response=q)
    p.response_swag = True                     # the whole swag comes back, device tensors included
    return p, q


def _run_pipeline(lanes, frames=PIPE_FRAMES):
    p, q = _pipeline(lanes)
    # the overlay's output replaces ``images`` in the swag: keep what it was given
    element = p.pipeline_graph.get_node("DetectionOverlay").element
    inner, seen = element.process_frame, []

    def spy(stream, images, *args, **kw):
        seen.append(images.clone())
        return inner(stream, images, *args, **kw)

    element.process_frame = spy
    outs = []
    for i in range(frames):
        p.process_frame({"stream_id": "c", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        torch.cuda.synchronize()               # buffers are reused per lane: copy before the next frame
        outs.append({"source": seen[i], "images": swag["images"].clone(), "det": swag["detections"].clone(),
                     "count": swag["counts"].clone(), "ids": swag["track_ids"].clone(),
                     "hits": swag["track_hits"].clone(), "labels": swag["labels"].clone()})
    assert p.share["gpu_lanes"] == lanes and len(seen) == frames
    return outs


def test_track_pipeline_matches_direct_calls(native):
    from aiko_services_amd.models.yolov8 import YOLOv8
    from aiko_services_amd.ops.overlay import default_font, default_palette, draw_detections, pack_names
    from aiko_services_amd.ops.track import new_state, track_detections
    one = _run_pipeline(1)
    yolo = YOLOv8(scale="n", seed=0, device="cuda", conf=PIPE_CONF)
    font, gw = default_font()
    names, font, palette = pack_names([f"#{i}" for i in range(1000)], 16).cuda(), font.cuda(), default_palette(20).cuda()
    state = new_state(2, PIPE_TRACKS, "cuda")
    for i, o in enumerate(one):
        det, count = yolo.detect(o["source"])
        ids, hits, labels, state = track_detections(det, count, state, PIPE_K, max_age=PIPE_MAX_AGE)
        direct = draw_detections(o["source"], det, count, PIPE_K, names, font, palette, labels=labels, glyph_width=gw)
        torch.cuda.synchronize()
        assert torch.equal(o["det"], det) and torch.equal(o["count"], count), i
        assert torch.equal(o["ids"], ids) and torch.equal(o["hits"], hits) and torch.equal(o["labels"], labels), i
        assert torch.equal(o["images"], direct), i
    all_ids, all_hits = torch.stack([o["ids"] for o in one]).cpu(), torch.stack([o["hits"] for o in one]).cpu()
    print(f"track pipeline: conf {PIPE_CONF}: ids per frame {all_ids.tolist()}, hits {all_hits.tolist()}")
    # the comparison means something only if a track is matched again AND slots are left empty
    assert (all_hits >= 2).any() and (all_ids == 0).any()
    two = _run_pipeline(2)
    for a, b in zip(one, two):
        for key in ("source", "images", "det", "count", "ids", "hits", "labels"):
            assert torch.equal(a[key], b[key]), key


def test_track_results_and_overlay_diagnostics(native):
    from aiko_services_amd.pipeline.stream import StreamEvent
    p, q = _pipeline(1, sink=True)
    for i in range(2):
        p.process_frame({"stream_id": "c", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        host = swag["tracks"].wait()
        assert all(t.is_pinned() for t in host.values())
        for key, name in (("det", "detections"), ("count", "counts"), ("ids", "track_ids"), ("hits", "track_hits")):
            assert host[key].device.type == "cpu" and torch.equal(host[key], swag[name].cpu()), key
    assert (host["ids"] > 0).any()
    overlay = p.pipeline_graph.get_node("DetectionOverlay").element
    images = torch.zeros(2, 240, 320, 3, dtype=torch.uint8, device="cuda")
    det, count, labels = swag["detections"], swag["counts"], swag["labels"]
    logits = torch.zeros(2 * PIPE_K, 1000, dtype=torch.bfloat16, device="cuda")
    event, out = overlay.process_frame(None, images, det, count, labels=labels)
    assert event == StreamEvent.OKAY
    event, out = overlay.process_frame(None, images, det, count, logits=logits, labels=labels)
    assert event == StreamEvent.ERROR and "labels and logits" in out["diagnostic"]
    event, out = overlay.process_frame(None, images, det, count, labels=labels[:-1])
    assert event == StreamEvent.ERROR and "labels int32" in out["diagnostic"]
    torch.cuda.synchronize()
