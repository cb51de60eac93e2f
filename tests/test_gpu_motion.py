"""The motion kernels (``ops.motion.motion_detect``, motion_ops.hip) against the CPU reference, bit
for bit and step by step, on the scenes of motion_scenes.py; the labelling's worst cases; then the
elements in the example pipeline against direct calls."""
import json
import queue
from pathlib import Path

import pytest
import torch

import motion_scenes as S
from kernel_guard import guarded
from motion_scenes import B, H

pytestmark = pytest.mark.gpu

NAMES = ("det", "count", "mask", "cells", "bg", "seen")
CONFIGS = [(cell, width, variant) for cell in S.CELLS for width in S.WIDTHS for variant in sorted(S.VARIANTS)]


def _flat(step):
    det, count, mask, cells, state = step
    return [t.cpu() for t in (det, count, mask, cells, *state)]


def _assert_step(got, want, where):
    for name, g, w in zip(NAMES, _flat(got), _flat(want)):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), f"{where}: {name}\n{g}\n{w}"


def _cuda_state(state):
    from aiko_services_amd.ops.motion import MotionState
    return MotionState(*(t.cuda() for t in state))


@pytest.mark.parametrize("cell,width,variant", CONFIGS)
def test_every_step_equals_reference(native, cell, width, variant):
    from aiko_services_amd.ops.motion import motion_detect
    scene, want = S.scene(cell, width, variant), S.reference(cell, width, variant)
    state = _cuda_state(scene.state0)
    for t, frames in enumerate(scene.frames):
        got = motion_detect(frames.cuda(), state, **scene.kw)
        torch.cuda.synchronize()
        _assert_step(got, want[t], f"cell {cell}, width {width}, {variant}, frame {t}")
        state = got[4]


def test_device_side_state_under_graph_replay(native):
    """Two steps in one graph, ping-ponging two states: a -> b -> a."""
    from aiko_services_amd.ops.motion import motion_detect, new_state
    cell, width = 16, S.W4
    scene, want = S.scene(cell, width, "base"), S.reference(cell, width, "base")
    kw = scene.kw
    gh, gw = S.grid(cell, width)
    frames = [torch.empty_like(scene.frames[0], device="cuda") for _ in range(2)]
    states = [new_state(B, H, width, cell, "cuda") for _ in range(2)]
    outs = [(torch.empty(B, kw["max_det"], 6, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"),
             torch.empty(B, gh, gw, dtype=torch.uint8, device="cuda"),
             torch.empty(B, dtype=torch.int32, device="cuda")) for _ in range(2)]

    def pair():
        for i in range(2):
            det, count, mask, cells = outs[i]
            motion_detect(frames[i], states[i], state_out=states[1 - i], det=det, count=count, mask=mask,
                          cells=cells, **kw)

    for f, src in zip(frames, scene.frames):
        f.copy_(src)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair()
    for dst, src in zip(states[0], scene.state0):
        dst.copy_(src)
    for t in range(0, 6, 2):
        for i in range(2):
            frames[i].copy_(scene.frames[t + i])
            for x in (*outs[i], *states[1]):                # poison: every element must be rewritten
                x.view(torch.uint8).fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        # the first step's state_out was read and then left alone: it is still frame t's
        _assert_step((*outs[0], states[1]), want[t], f"replay, frame {t}")
        _assert_step((*outs[1], states[0]), want[t + 1], f"replay, frame {t + 1}")


@pytest.mark.parametrize("cell,width", [(8, S.W), (16, S.W4), (32, S.W)])
def test_guard_bands_and_no_poison_left(native, cell, width):
    from aiko_services_amd.ops.motion import MotionState, motion_detect
    scene, want = S.scene(cell, width, "base"), S.reference(cell, width, "base")
    kw = scene.kw
    gh, gw = S.grid(cell, width)
    at = 3                                                  # mid-scene: a learnt background, regions in two cameras
    before = want[at - 1][4]
    checks = []

    def g(shape, dtype, values=None, name=""):
        view, check = guarded(shape, dtype, "cuda", values=values, name=name)
        checks.append(check)
        return view

    gf = g(scene.frames[at].shape, torch.uint8, scene.frames[at], "frames")
    gin = MotionState(g((B, gh, gw), torch.int32, before.bg, "bg"), g((B,), torch.int32, before.seen, "seen"))
    gout = MotionState(g((B, gh, gw), torch.int32, name="bg_out"), g((B,), torch.int32, name="seen_out"))
    det, count = g((B, kw["max_det"], 6), torch.float32, name="det"), g((B,), torch.int32, name="count")
    mask, cells = g((B, gh, gw), torch.uint8, name="mask"), g((B,), torch.int32, name="cells")
    motion_detect(gf, gin, state_out=gout, det=det, count=count, mask=mask, cells=cells, **kw)
    torch.cuda.synchronize()
    for check in checks:
        check()
    _assert_step((det, count, mask, cells, gout), want[at], "guarded")
    # no element of any output kept its poison (0xA5 bytes, the fp32 NaN): rows past count and the
    # whole of state_out included
    for x in (count, cells, gout.bg, gout.seen):
        assert not (x.view(torch.uint8).view(-1, 4) == 0xA5).all(1).any()
    assert torch.isfinite(det).all() and int(mask.max()) <= 1
    assert int(count.min()) < kw["max_det"]
    assert all(not det[b, int(count[b]):].any() for b in range(B))
    # the inputs are only read
    assert torch.equal(gin.bg.cpu(), before.bg) and torch.equal(gin.seen.cpu(), before.seen)
    assert torch.equal(gf.cpu(), scene.frames[at])


def test_refusals(native):
    from aiko_services_amd.ops.motion import MotionState, motion_detect, new_state
    scene = S.scene(16, S.W, "base")
    frames = scene.frames[1].cuda()
    state = new_state(B, H, S.W, 16, "cuda")
    gh, gw = S.grid(16)

    def refuse(match, frames=frames, state=state, error=RuntimeError, **kw):
        with pytest.raises(error, match=match):
            motion_detect(frames, state, **{"cell": 16, **kw})

    refuse("frames uint8", frames=frames.float())
    refuse("frames uint8", frames=frames[..., :2].contiguous())
    refuse("frames uint8", frames=torch.zeros(B, H, 2 * S.W, 3, dtype=torch.uint8, device="cuda")[:, :, ::2])
    refuse("state bg int32", state=MotionState(state.bg.float(), state.seen))
    refuse("state bg int32", state=MotionState(state.bg, state.seen.long()))
    refuse("state bg int32", state=new_state(B + 1, H, S.W, 16, "cuda"))
    refuse("state bg int32", state=new_state(B, H, S.W, 8, "cuda"))
    refuse("state bg int32", state=MotionState(torch.zeros(B, gh, 2 * gw, dtype=torch.int32, device="cuda")[:, :, ::2],
                                                state.seen))
    refuse("state_out bg int32", state_out=new_state(B, H + 16, S.W, 16, "cuda"))
    refuse("state_out bg int32", state_out=MotionState(state.bg.clone(), state.seen.clone().long()))
    refuse("det fp32", det=torch.empty(B, 16, 6, dtype=torch.float64, device="cuda"))
    refuse("det fp32", det=torch.empty(B + 1, 16, 6, device="cuda"))
    refuse("count and cells int32", count=torch.empty(B, dtype=torch.int64, device="cuda"))
    refuse("count and cells int32", cells=torch.empty(B + 1, dtype=torch.int32, device="cuda"))
    refuse("mask uint8", mask=torch.empty(B, gh, gw, dtype=torch.int8, device="cuda"))
    refuse("mask uint8", mask=torch.empty(B, gh, gw + 1, dtype=torch.uint8, device="cuda"))
    refuse("GPU tensor", frames=frames.cpu())
    refuse("GPU tensor", state=new_state(B, H, S.W, 16, "cpu"))
    refuse("GPU tensor", state_out=new_state(B, H, S.W, 16, "cpu"))
    refuse("GPU tensor", det=torch.empty(B, 16, 6))
    if torch.cuda.device_count() > 1:
        refuse("device", state=new_state(B, H, S.W, 16, "cuda:1"))
    # state_out must be another allocation; no output over an input or another output
    refuse("bg_out and bg overlap", state_out=state)
    refuse("seen_out and seen overlap", state_out=MotionState(state.bg.clone(), state.seen))
    shared = torch.zeros(2 * B, dtype=torch.int32, device="cuda")
    refuse("cells and count overlap", count=shared[:B], cells=shared[B - 1:2 * B - 1])
    refuse("count and seen overlap", state=MotionState(state.bg, shared[:B]), count=shared[:B])
    # values: Python errors
    for cell in (4, 12, 64):
        refuse("cell", error=ValueError, cell=cell)
    for max_det in (0, 65, -1):
        refuse("max_det", error=ValueError, max_det=max_det)
    refuse("max_det", error=ValueError, max_det=16, det=torch.empty(B, 8, 6, device="cuda"))
    refuse("threshold", error=ValueError, threshold=256)
    refuse("learn_shift", error=ValueError, learn_shift=9)
    refuse("warmup", error=ValueError, warmup=0)
    refuse("min_cells", error=ValueError, min_cells=0)
    # the operator's own bounds, past the Python layer
    with pytest.raises(RuntimeError, match="1 <= max_det <= 64"):
        torch.ops.aiko.motion_detect_out(frames, state.bg, state.seen, 16, 12, 4, True, 1, 2, state.bg.clone(),
                                         state.seen.clone(), torch.empty(B, 65, 6, device="cuda"),
                                         torch.empty(B, dtype=torch.int32, device="cuda"),
                                         torch.empty(B, gh, gw, dtype=torch.uint8, device="cuda"),
                                         torch.empty(B, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="grid limit"):                  # 65536 frames: past the launch grid
        torch.ops.aiko.motion_detect_out(torch.zeros(65536, 1, 1, 3, dtype=torch.uint8, device="cuda"), state.bg,
                                         state.seen, 16, 12, 4, True, 1, 2, state.bg.clone(), state.seen.clone(),
                                         torch.empty(B, 16, 6, device="cuda"),
                                         torch.empty(B, dtype=torch.int32, device="cuda"),
                                         torch.empty(B, gh, gw, dtype=torch.uint8, device="cuda"),
                                         torch.empty(B, dtype=torch.int32, device="cuda"))
    # the grid limits: 1080p at cell 8 is 135 x 240 = 32400 cells; 257 columns; 257 rows
    for h, w in ((1080, 1920), (8, 2056), (2056, 8)):
        big = torch.zeros(1, h, w, 3, dtype=torch.uint8, device="cuda")
        refuse("exceeds the limits", frames=big, state=new_state(1, h, w, 8, "cuda"), cell=8)
    # inside them: 1080p at cell 16, and the extremes of every parameter
    big = torch.zeros(1, 1080, 1920, 3, dtype=torch.uint8, device="cuda")
    out = motion_detect(big, new_state(1, 1080, 1920, 16, "cuda"), cell=16)
    motion_detect(frames, state, cell=16, threshold=0, learn_shift=0, max_det=64, warmup=2 ** 31 - 1)
    motion_detect(frames, state, cell=16, threshold=255, learn_shift=8, max_det=1, min_cells=2 ** 31 - 1)
    torch.cuda.synchronize()
    assert out[2].shape == (1, 68, 120) and int(out[4].seen[0]) == 1


# ---- the labelling's worst cases ------------------------------------------------------------

@pytest.mark.parametrize("name", ["serpentine", "serpentine_t", "checkerboard", "all", "empty"])
def test_labelling_worst_cases(native, name):
    """One frame on the full 128 x 128 grid: the serpentine needs the most rounds (128 in a CPU
    prototype of the scheme), the checkerboard is one component only through corners."""
    from aiko_services_amd.ops.motion import motion_detect
    from aiko_services_amd.ops.reference import motion_detect_ref
    mask = S.worst_masks()[name]
    frame, state = S.worst_case(mask)
    kw = dict(cell=S.WORST_CELL, threshold=S.THRESHOLD, min_cells=2, max_det=4)
    want = motion_detect_ref(frame, state, **kw)
    assert torch.equal(want[2][0].bool(), mask) and int(want[1][0]) == (0 if name == "empty" else 1)
    got = motion_detect(frame.cuda(), _cuda_state(state), **kw)
    torch.cuda.synchronize()
    _assert_step(got, want, name)


def test_many_small_components_fill_every_row(native):
    """Isolated pairs all over the 128 x 128 grid: 64 x 42 components of area 2, max_det 64 rows out,
    in label order."""
    from aiko_services_amd.ops.motion import motion_detect
    from aiko_services_amd.ops.reference import motion_detect_ref
    n = S.WORST_SIDE // S.WORST_CELL
    mask = torch.zeros(n, n, dtype=torch.bool)
    mask[0::2, 0::3] = True
    mask[0::2, 1::3] = True
    mask[:, n - 2:] = False
    frame, state = S.worst_case(mask)
    kw = dict(cell=S.WORST_CELL, threshold=S.THRESHOLD, min_cells=2, max_det=64)
    want = motion_detect_ref(frame, state, **kw)
    assert int(want[1][0]) == 64 and int(want[3][0]) == int(mask.sum()) and bool((want[0][0, :, 4] == 1).all())
    got = motion_detect(frame.cuda(), _cuda_state(state), **kw)
    torch.cuda.synchronize()
    _assert_step(got, want, "pairs")


# ---- the example pipeline -------------------------------------------------------------------

# SyntheticFrames slots are independent random pixels: at cell 16 two slots' cell means differ by a
# few luma levels, so threshold 1 is what makes the reference itself report moving cells (asserted
# below).  The frame pool rotates 4 batches: frames 4 and 5 show frames 0 and 1 again.
PIPE_THRESHOLD = 1
PIPE_K = 8
PIPE_MAX_DET = 16
PIPE_FRAMES = 6
PIPE_B, PIPE_H, PIPE_W = 2, 240, 320
EXAMPLE = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/yolo/yolo_motion_gpu.json"


def _definition(lanes, sink=False):
    d = json.loads(EXAMPLE.read_text())
    d["parameters"]["gpu_lanes"] = lanes
    by_name = {e["name"]: e for e in d["elements"]}
    by_name["SyntheticFrames"]["parameters"].update(batch=PIPE_B, height=PIPE_H, width=PIPE_W, pool=4)
    by_name["MotionDetector"]["parameters"].update(threshold=PIPE_THRESHOLD, max_det=PIPE_MAX_DET)
    by_name["DetectionTracker"]["parameters"].update(rois=PIPE_K)
    by_name["DetectionOverlay"]["parameters"].update(rois=PIPE_K)
    if sink:
        d["graph"] = ["(SyntheticFrames MotionDetector DetectionTracker DetectionOverlay MotionResults)"]
        tensor = lambda name: {"name": name, "type": "tensor"}  # noqa: E731
        d["elements"].append({"name": "MotionResults",
                              "input": [tensor("detections"), tensor("counts"), tensor("motion_mask"),
                                        tensor("motion_cells")],
                              "output": [{"name": "motion", "type": "result"}], "parameters": {},
                              "deploy": {"local": {"module": "aiko_services_amd.elements.gpu.motion"}}})
    return d


def _pipeline(lanes, sink=False):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<motion>", parse_pipeline_definition_dict(_definition(lanes, sink)),
                                     None, None, "c", [], 0, None, 60, queue_response=q)
    p.response_swag = True                     # the whole swag comes back, device tensors included
    return p, q


def _run_pipeline(lanes, frames=PIPE_FRAMES):
    p, q = _pipeline(lanes)
    # the overlay's output replaces ``images`` in the swag: keep what the detector was given
    element = p.pipeline_graph.get_node("MotionDetector").element
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
                     "count": swag["counts"].clone(), "mask": swag["motion_mask"].clone(),
                     "cells": swag["motion_cells"].clone(), "ids": swag["track_ids"].clone(),
                     "labels": swag["labels"].clone()})
    assert p.share["gpu_lanes"] == lanes and len(seen) == frames
    return outs


def test_motion_pipeline_matches_direct_calls(native):
    from aiko_services_amd.ops.motion import motion_detect, new_state
    from aiko_services_amd.ops.overlay import default_font, default_palette, draw_detections, pack_names
    from aiko_services_amd.ops.reference import motion_detect_ref
    from aiko_services_amd.ops.track import new_state as new_tracks, track_detections
    one = _run_pipeline(1)
    font, gw = default_font()
    names, font, palette = pack_names([f"#{i}" for i in range(1000)], 16).cuda(), font.cuda(), default_palette(20).cuda()
    kw = dict(cell=16, threshold=PIPE_THRESHOLD, learn_shift=4, learn_moving=True, warmup=1, min_cells=2,
              max_det=PIPE_MAX_DET)
    state, ref_state = new_state(PIPE_B, PIPE_H, PIPE_W, 16, "cuda"), new_state(PIPE_B, PIPE_H, PIPE_W, 16, "cpu")
    tracks = new_tracks(PIPE_B, 32, "cuda")
    moving = 0
    for i, o in enumerate(one):
        det, count, mask, cells, state = motion_detect(o["source"], state, **kw)
        ids, hits, labels, tracks = track_detections(det, count, tracks, PIPE_K)
        direct = draw_detections(o["source"], det, count, PIPE_K, names, font, palette, labels=labels, glyph_width=gw)
        want = motion_detect_ref(o["source"].cpu(), ref_state, **kw)
        ref_state = want[4]
        torch.cuda.synchronize()
        _assert_step((det, count, mask, cells, state), want, f"direct, frame {i}")
        assert torch.equal(o["det"], det) and torch.equal(o["count"], count), i
        assert torch.equal(o["mask"], mask) and torch.equal(o["cells"], cells), i
        assert torch.equal(o["ids"], ids) and torch.equal(o["labels"], labels), i
        assert torch.equal(o["images"], direct), i
        moving += int(want[3].sum())
        if i > 0:                                           # the reference itself reports motion, and rows
            assert int(want[3].min()) > 0 and int(want[1].min()) > 0, i
    print(f"motion pipeline: threshold {PIPE_THRESHOLD}: {moving} moving cells over {PIPE_FRAMES} frames, "
          f"counts {[o['count'].tolist() for o in one]}")
    assert any(bool((o["ids"] > 0).any()) for o in one) and any(not torch.equal(o["images"], o["source"]) for o in one)
    two = _run_pipeline(2)
    for a, b in zip(one, two):
        for key in ("source", "images", "det", "count", "mask", "cells", "ids", "labels"):
            assert torch.equal(a[key], b[key]), key


def test_motion_results_and_diagnostics(native):
    from aiko_services_amd.pipeline.stream import StreamEvent
    p, q = _pipeline(1, sink=True)
    for i in range(2):
        p.process_frame({"stream_id": "c", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        host = swag["motion"].wait()
        assert all(t.is_pinned() for t in host.values())
        for key, name in (("det", "detections"), ("count", "counts"), ("mask", "motion_mask"),
                          ("cells", "motion_cells")):
            assert host[key].device.type == "cpu" and torch.equal(host[key], swag[name].cpu()), key
    assert int(host["cells"].min()) > 0 and int(host["count"].min()) > 0
    element = p.pipeline_graph.get_node("MotionDetector").element
    good = torch.zeros(PIPE_B, PIPE_H, PIPE_W, 3, dtype=torch.uint8, device="cuda")
    event, out = element.process_frame(None, good)
    assert event == StreamEvent.OKAY and out["images"] is good
    # another geometry: the state starts again
    event, out = element.process_frame(None, good[:, :100].contiguous())
    torch.cuda.synchronize()
    assert event == StreamEvent.OKAY and int(out["motion_cells"].sum()) == 0 and out["motion_mask"].shape == (PIPE_B, 7, 20)
    for bad, text in ((good.float(), "images uint8"), (good[..., :2], "images uint8"), (good.cpu(), "images uint8"),
                      (None, "images uint8"),
                      (torch.zeros(1, 16, 16 * 256, 3, dtype=torch.uint8, device="cuda"), "past the limits")):
        event, out = element.process_frame(None, bad)
        assert event == StreamEvent.ERROR and text in out["diagnostic"], out
    torch.cuda.synchronize()
