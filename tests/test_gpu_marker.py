"""The marker kernels (``ops.marker.detect_markers``, marker_ops.hip) against the CPU reference, bit
for bit, on the scenes of marker_scenes.py, both widths and cells 4 and 8; under hipGraph replay;
between guard bands; the operator's refusals; then the elements in the example pipeline against
direct calls."""
import json
import queue
from pathlib import Path

import numpy as np
import pytest
import torch

import marker_scenes as S
from kernel_guard import guarded
from marker_scenes import B, H

pytestmark = pytest.mark.gpu

NAMES = ("det", "count", "corners", "ids", "cands", "mask")
CONFIGS = [(name, width, cell) for name in S.NAMES for width in S.WIDTHS for cell in S.CELLS]


def _assert_equal(got, want, where):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), f"{where}: {name}\n{g}\n{w}"


def _kw(name, width, cell):
    return {**S.scene(name, width).kw, "cell": cell}


def _buffers(kw, width, device="cuda", make=None):
    from aiko_services_amd.ops.marker import work_size
    gh, gw = S.grid(kw["cell"], width)
    k, i32 = kw["max_det"], torch.int32
    specs = dict(det=((B, k, 6), torch.float32), count=((B,), i32), corners=((B, k, 4, 2), i32), ids=((B, k), i32),
                 cands=((B,), i32), mask=((B, gh, gw), torch.uint8), work=((work_size(B, H, width),), i32))
    make = make or (lambda shape, dtype, name: torch.empty(shape, dtype=dtype, device=device))
    return {name: make(shape, dtype, name) for name, (shape, dtype) in specs.items()}


@pytest.mark.parametrize("name,width,cell", CONFIGS)
def test_every_scene_equals_reference(native, name, width, cell):
    from aiko_services_amd.ops.marker import detect_markers
    got = detect_markers(S.scene(name, width).frames.cuda(), **_kw(name, width, cell))
    torch.cuda.synchronize()
    _assert_equal(got, S.reference(name, width, cell), f"{name}, width {width}, cell {cell}")


def test_cell_16_and_both_dictionaries_on_one_frame(native):
    """The third cell size (two waves share a cell row in the mask pass), and a frame of original
    markers read as payload16: whatever that finds, the kernels find the same."""
    from aiko_services_amd.ops.marker import detect_markers
    from aiko_services_amd.ops.reference import detect_markers_ref
    for name, width, kw in (("large", S.W_ODD, dict(cell=16)), ("upright", S.W, dict(cell=16, min_side=16)),
                            ("angles_a", S.W, dict(dictionary="payload16")),
                            ("worst", S.W_ODD, dict(contrast=1, min_side=1, max_cand=64, max_det=64)),
                            ("negatives", S.W, dict(contrast=255))):
        frames = S.scene(name, width).frames
        kw = {**S.scene(name, width).kw, **kw}
        got = detect_markers(frames.cuda(), **kw)
        torch.cuda.synchronize()
        _assert_equal(got, detect_markers_ref(frames, **kw), f"{name}, {kw}")


@pytest.mark.parametrize("width", S.WIDTHS)
def test_graph_replay_rewrites_every_output(native, width):
    from aiko_services_amd.ops.marker import detect_markers
    names = ("angles_a", "caps", "worst", "negatives")      # one dictionary, two sets of caps
    frames = torch.empty_like(S.scene(names[0], width).frames, device="cuda")
    for kw_of in ("angles_a", "caps"):
        kw = _kw(kw_of, width, 4)
        out = _buffers(kw, width)
        frames.copy_(S.scene(names[0], width).frames)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            detect_markers(frames, **kw, **out)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            detect_markers(frames, **kw, **out)
        for name in names:
            from aiko_services_amd.ops.reference import detect_markers_ref
            scene = S.scene(name, width)
            frames.copy_(scene.frames)
            for x in out.values():                          # poison: every element must be rewritten
                x.view(torch.uint8).fill_(0x5A)
            graph.replay()
            torch.cuda.synchronize()
            want = S.reference(name, width, 4) if scene.kw == {**kw, "cell": 4} else detect_markers_ref(scene.frames, **kw)
            _assert_equal([out[n] for n in NAMES], want, f"replay, {name} with the caps of {kw_of}, width {width}")


@pytest.mark.parametrize("name,width,cell", [("angles_b", S.W, 4), ("edges", S.W_ODD, 4), ("worst", S.W_ODD, 8),
                                             ("caps", S.W, 8)])
def test_guard_bands_and_no_poison_left(native, name, width, cell):
    from aiko_services_amd.ops.marker import detect_markers
    scene, kw = S.scene(name, width), _kw(name, width, cell)
    checks = []

    def g(shape, dtype, label, values=None):
        view, check = guarded(shape, dtype, "cuda", values=values, name=label)
        checks.append(check)
        return view

    gf = g(scene.frames.shape, torch.uint8, "frames", scene.frames)
    out = _buffers(kw, width, make=g)
    detect_markers(gf, **kw, **out)
    torch.cuda.synchronize()
    for check in checks:
        check()
    want = S.reference(name, width, cell)
    _assert_equal([out[n] for n in NAMES], want, "guarded")
    plain = detect_markers(scene.frames.cuda(), **kw)
    torch.cuda.synchronize()
    _assert_equal([out[n] for n in NAMES], [t.cpu() for t in plain], "guarded against unguarded")
    # no element of any output kept its poison (0xA5 bytes, the fp32 NaN), rows past count included
    for x in (out["count"], out["cands"], out["corners"], out["ids"]):
        assert not (x.contiguous().view(torch.uint8).view(-1, 4) == 0xA5).all(1).any()
    assert torch.isfinite(out["det"]).all() and int(out["mask"].max()) <= 1
    assert int(out["count"].min()) < kw["max_det"]
    for b in range(B):
        n = int(out["count"][b])
        assert not out["det"][b, n:].any() and not out["corners"][b, n:].any() and bool((out["ids"][b, n:] == -1).all())
    assert torch.equal(gf.cpu(), scene.frames)              # the frames are only read


def test_refusals(native):
    from aiko_services_amd.ops.marker import detect_markers, work_size
    width = S.W
    frames = S.scene("upright", width).frames.cuda()
    gh, gw = S.grid(4, width)

    def refuse(match, frames=frames, error=RuntimeError, **kw):
        with pytest.raises(error, match=match):
            detect_markers(frames, **kw)

    dev, i32 = "cuda", torch.int32
    refuse("frames uint8", frames=frames.float())
    refuse("frames uint8", frames=frames[..., :2].contiguous())
    refuse("frames uint8", frames=torch.zeros(B, H, 2 * width, 3, dtype=torch.uint8, device=dev)[:, :, ::2])
    refuse("det fp32", det=torch.empty(B, 16, 6, dtype=torch.float64, device=dev))
    refuse("det fp32", det=torch.empty(B + 1, 16, 6, device=dev))
    refuse("det fp32", det=torch.empty(B, 16, 12, device=dev)[:, :, ::2])
    refuse("count and cands int32", count=torch.empty(B, dtype=torch.int64, device=dev))
    refuse("count and cands int32", cands=torch.empty(B + 1, dtype=i32, device=dev))
    refuse("corners int32", corners=torch.empty(B, 16, 4, 2, dtype=torch.float32, device=dev))
    refuse("corners int32", corners=torch.empty(B, 8, 4, 2, dtype=i32, device=dev))
    refuse("ids int32", ids=torch.empty(B, 16, dtype=torch.int64, device=dev))
    refuse("ids int32", ids=torch.empty(B, 17, dtype=i32, device=dev))
    refuse("mask uint8", mask=torch.empty(B, gh, gw, dtype=torch.int8, device=dev))
    refuse("mask uint8", mask=torch.empty(B, gh, gw + 1, dtype=torch.uint8, device=dev))
    refuse("work int32", work=torch.empty(work_size(B, H, width) - 1, dtype=i32, device=dev))
    refuse("work int32", work=torch.empty(work_size(B, H, width), dtype=torch.float32, device=dev))
    refuse("GPU tensor", frames=frames.cpu(), det=torch.empty(B, 16, 6, device=dev))
    refuse("CPU", frames=frames.cpu())                      # nothing on the device: no such operator
    refuse("GPU tensor", det=torch.empty(B, 16, 6))
    refuse("GPU tensor", work=torch.empty(work_size(B, H, width), dtype=i32))
    if torch.cuda.device_count() > 1:
        refuse("device", count=torch.empty(B, dtype=i32, device="cuda:1"))
    # no output over the frames or another output
    shared = torch.zeros(2 * B, dtype=i32, device=dev)
    refuse("cands and count overlap", count=shared[:B], cands=shared[B - 1:2 * B - 1])
    both = torch.zeros(B * 16 * 9, dtype=i32, device=dev)
    refuse("ids and corners overlap", corners=both[:B * 16 * 8].view(B, 16, 4, 2), ids=both[B * 16 * 7:B * 16 * 8].view(B, 16))
    refuse("mask and frames overlap", mask=frames.view(-1)[:B * gh * gw].view(B, gh, gw))
    # values: Python errors
    for cell in (2, 12, 32):
        refuse("cell", error=ValueError, cell=cell)
    for max_det in (0, 65, -1):
        refuse("max_det", error=ValueError, max_det=max_det)
    refuse("max_det", error=ValueError, max_det=16, det=torch.empty(B, 8, 6, device=dev))
    refuse("max_cand", error=ValueError, max_cand=65)
    refuse("contrast", error=ValueError, contrast=0)
    refuse("min_side", error=ValueError, min_side=0)
    refuse("dictionary", error=ValueError, dictionary="DICT_4X4_50")
    # the operator's own bounds, past the Python layer
    out = _buffers(dict(S.BASE), width)
    args = [out[n] for n in (*NAMES, "work")]
    for bad, match in (((5, 4, 64, 24, 32, 7), "modules"), ((7, 2, 64, 24, 32, 7), "cell in"),
                       ((7, 4, 256, 24, 32, 7), "contrast"), ((7, 4, 64, 0, 32, 7), "min_side"),
                       ((7, 4, 64, 24, 65, 7), "max_cand"), ((7, 4, 64, 24, 32, 8), "passes")):
        with pytest.raises(RuntimeError, match=match):
            torch.ops.aiko.marker_detect_out(frames, *bad, *args)
    with pytest.raises(RuntimeError, match="1 <= max_det <= 64"):
        torch.ops.aiko.marker_detect_out(frames, 7, 4, 64, 24, 32, 7, torch.empty(B, 65, 6, device=dev), *args[1:])
    # the grid limit: 720p at cell 4; a side above 4096
    refuse("exceeds the limit", frames=torch.zeros(1, 720, 1280, 3, dtype=torch.uint8, device=dev))
    refuse("exceed the frame limits", frames=torch.zeros(1, 8, 4097, 3, dtype=torch.uint8, device=dev), cell=16)
    refuse("exceed the frame limits", frames=torch.zeros(1, 4097, 8, 3, dtype=torch.uint8, device=dev), cell=16)
    # inside them: 480 x 640 at cell 4, 1080p at cell 8 (blank: the labelling has nothing to do), 8 x 4096
    for h, w, cell in ((480, 640, 4), (1080, 1920, 8), (8, 4096, 16)):
        big = torch.full((1, h, w, 3), 200, dtype=torch.uint8, device=dev)
        det, count, corners, ids, cands, mask = detect_markers(big, cell=cell, max_cand=64, max_det=64, contrast=255)
        torch.cuda.synchronize()
        assert mask.shape == (1, -(-h // cell), -(-w // cell)) and int(count[0]) == 0 and not mask.any()
        assert bool((ids == -1).all()) and not det.any()


def limit_case(h, w, cell, side):
    """(frames uint8 [1, h, w, 3], the reference's result): two markers over a band of 16-pixel
    texture, which is one huge component and a few small ones."""
    from aiko_services_amd.ops.reference import detect_markers_ref
    gray = np.full((h, w), float(S.WHITE))
    rng = np.random.default_rng(5)
    band = h - 3 * h // 4
    gray[h - band:, :] = np.kron(rng.integers(0, 2, (band // 16 + 1, w // 16 + 1)),
                                 np.ones((16, 16)))[:band, :w] * (S.WHITE - S.BLACK) + S.BLACK
    S.paint(gray, S.module_grid("original", 345), S.square(w // 4, h // 3, side, 25))
    S.paint(gray, S.module_grid("original", 678), S.square(w - 100, h // 3, side, 110, squeeze=0.7))
    frames = S.light(gray)[None]
    return frames, detect_markers_ref(frames, cell=cell)


@pytest.mark.parametrize("h,w,cell,side", [(480, 640, 4, 70), (1080, 1920, 8, 160)])
def test_a_marker_in_a_frame_at_the_grid_limit(native, h, w, cell, side):
    """480 x 640 at cell 4 and 1080p at cell 8, the dynamic LDS above 64 KB: against the reference."""
    from aiko_services_amd.ops.marker import detect_markers
    frames, want = limit_case(h, w, cell, side)
    assert sorted(want[3][0, :2].tolist()) == [345, 678] and int(want[1][0]) == 2 and int(want[4][0]) > 2
    got = detect_markers(frames.cuda(), cell=cell)
    torch.cuda.synchronize()
    _assert_equal(got, want, f"{h} x {w}, cell {cell}")


# ---- the example pipeline -------------------------------------------------------------------

EXAMPLE = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/aruco_marker/aruco_pipeline_gpu.json"
PIPE_SCENES = ("angles_a", "large")
PIPE_FRAMES = 4


def _pipeline(lanes):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    d = json.loads(EXAMPLE.read_text())
    d["parameters"]["gpu_lanes"] = lanes
    by_name = {e["name"]: e for e in d["elements"]}
    by_name["SyntheticFrames"]["parameters"].update(batch=B, height=H, width=S.W, pool=len(PIPE_SCENES))
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<marker>", parse_pipeline_definition_dict(d), None, None, "c", [], 0, None, 60,
                                     queue_response=q)
    p.response_swag = True                     # the whole swag comes back, device tensors included
    source = p.pipeline_graph.get_node("SyntheticFrames").element
    source._ensure_pool(False)                 # the slots hold the scenes' frames instead of noise
    for slot, name in enumerate(PIPE_SCENES):
        source.frame_pool.view(slot, source._shape, torch.uint8).copy_(S.scene(name).frames)
    torch.cuda.synchronize()
    return p, q


def _run_pipeline(lanes):
    p, q = _pipeline(lanes)
    element = p.pipeline_graph.get_node("MarkerDetector").element
    inner, seen = element.process_frame, []

    def spy(stream, images, *args, **kw):      # the overlay's output replaces ``images`` in the swag
        seen.append(images.clone())
        return inner(stream, images, *args, **kw)

    element.process_frame = spy
    outs = []
    for i in range(PIPE_FRAMES):
        p.process_frame({"stream_id": "c", "frame_id": i}, {})
        info, swag = q.get_nowait()
        assert info["state"] == 0, swag
        host = swag["markers"].wait()
        torch.cuda.synchronize()               # buffers are reused per lane: copy before the next frame
        outs.append({"source": seen[i], "images": swag["images"].clone(), "det": swag["detections"].clone(),
                     "count": swag["counts"].clone(), "corners": swag["marker_corners"].clone(),
                     "ids": swag["marker_ids"].clone(), "labels": swag["labels"].clone(),
                     "host": {k: v.clone() for k, v in host.items()}, "pinned": all(t.is_pinned() for t in host.values())})
    assert p.share["gpu_lanes"] == lanes and len(seen) == PIPE_FRAMES
    return p, outs


def test_marker_pipeline_matches_direct_calls(native):
    from aiko_services_amd.elements.gpu.marker import to_overlays
    from aiko_services_amd.ops.marker import detect_markers
    from aiko_services_amd.ops.overlay import default_font, default_palette, draw_detections, pack_names
    p, one = _run_pipeline(1)
    font, gw = default_font()
    names, font, palette = pack_names([f"#{i}" for i in range(1024)], 16).cuda(), font.cuda(), default_palette(20).cuda()
    found = 0
    for i, o in enumerate(one):
        by_frames = [n for n in PIPE_SCENES if torch.equal(S.scene(n).frames, o["source"].cpu())]
        assert len(by_frames) == 1, i
        want = S.reference(by_frames[0], S.W, 4)
        det, count, corners, ids, cands, mask = detect_markers(o["source"], dictionary="original")
        labels = (ids.clamp(min=0) % 1024).view(-1)
        direct = draw_detections(o["source"], det, count, 16, names, font, palette, labels=labels, glyph_width=gw)
        torch.cuda.synchronize()
        _assert_equal((det, count, corners, ids, cands, mask), want, f"direct, frame {i}")
        for key, t in (("det", det), ("count", count), ("corners", corners), ("ids", ids), ("labels", labels)):
            assert torch.equal(o[key], t), (i, key)
        assert torch.equal(o["images"], direct) and not torch.equal(o["images"], o["source"]), i
        assert o["pinned"]
        for key in ("det", "count", "corners", "ids"):
            assert o["host"][key].device.type == "cpu" and torch.equal(o["host"][key], o[key].cpu()), (i, key)
        # the host element's overlays, and its overlay element behind them
        overlays = to_overlays(o["host"])
        assert len(overlays) == B
        for b, overlay in enumerate(overlays):
            n = int(want[1][b])
            assert len(overlay["corners"]) == n and overlay["ids"].shape == (n, 1) and overlay["ids"].dtype == np.int32
            assert overlay["ids"].reshape(-1).tolist() == want[3][b, :n].tolist()
            for k, quad in enumerate(overlay["corners"]):
                assert quad.shape == (1, 4, 2) and quad.dtype == np.float32
                assert quad.reshape(4, 2).tolist() == want[2][b, k].tolist()
            found += n
        drawn = _host_overlay(o["source"].cpu().numpy(), overlays)
        assert all((drawn[b] != o["source"][b].cpu().numpy()).any() == (int(want[1][b]) > 0) for b in range(B)), i
    assert found >= 20
    _, two = _run_pipeline(2)
    for a, b in zip(one, two):
        for key in ("source", "images", "det", "count", "corners", "ids", "labels"):
            assert torch.equal(a[key], b[key]), key


def _host_overlay(images, overlays):
    """``ArucoMarkerOverlay.process_frame`` on the host, without a pipeline around it."""
    from aiko_services_amd.examples.aruco_marker.aruco import ArucoMarkerOverlay
    from aiko_services_amd.pipeline.stream import StreamEvent
    event, out = ArucoMarkerOverlay.process_frame(None, None, list(images), overlays)
    assert event == StreamEvent.OKAY and out["overlays"] is overlays
    return out["images"]


def test_marker_detector_diagnostics(native):
    from aiko_services_amd.pipeline.stream import StreamEvent
    p, q = _pipeline(1)
    element = p.pipeline_graph.get_node("MarkerDetector").element
    good = S.scene("upright").frames.cuda()
    event, out = element.process_frame(None, good)
    torch.cuda.synchronize()
    assert event == StreamEvent.OKAY and out["images"] is good and out["counts"].tolist() == [4, 1, 0]
    assert out["labels"].shape == (B * 16,) and out["labels"][:4].tolist() == [100, 107, 114, 121]
    assert out["labels"][16].item() == 1000 and not out["labels"][17:].any()
    # another geometry: other buffers
    event, other = element.process_frame(None, good[:, :100].contiguous())
    torch.cuda.synchronize()
    assert event == StreamEvent.OKAY and other["detections"] is not out["detections"]
    for bad, text in ((good.float(), "images uint8"), (good[..., :2], "images uint8"), (good.cpu(), "images uint8"),
                      (None, "images uint8"),
                      (torch.zeros(1, 720, 1280, 3, dtype=torch.uint8, device="cuda"), "past the limits"),
                      (torch.zeros(1, 8, 4100, 3, dtype=torch.uint8, device="cuda"), "past the limits")):
        event, out = element.process_frame(None, bad)
        assert event == StreamEvent.ERROR and text in out["diagnostic"], out
    torch.cuda.synchronize()
