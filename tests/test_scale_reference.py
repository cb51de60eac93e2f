"""The antialiased resize's rule on the CPU (``ops/scale.py``): ``scale_frames_ref`` byte for byte
against Pillow's ``Image.resize`` on the shared scenes (scale_scenes.py), against a second
formulation (dense coefficient matrices), the properties the rule states, the refusals of the plan
makers, and the host branch of ``ImageResize`` with and without ``filter``."""
import queue

import numpy as np
import pytest
import torch

import scale_scenes as S
from aiko_services_amd.ops import scale as Sc
from aiko_services_amd.ops.reference import scale_frames_ref, scale_pass_sums_ref


def pil_filter(name):
    from PIL import Image
    return {"box": Image.BOX, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING, "bicubic": Image.BICUBIC,
            "lanczos": Image.LANCZOS}[name]


@pytest.mark.parametrize("pair", S.PAIRS, ids=lambda p: "{}x{}-{}x{}".format(*p))
def test_equals_pillow(pair):
    """No allowance: every byte of every frame, all five filters, whole frame and box."""
    Image = pytest.importorskip("PIL.Image")
    h, w, ho, wo = pair
    for f in S.FILTER_NAMES:
        for boxed in (False, True):
            case = (pair, f, boxed)
            ref = S.reference(case).numpy()
            bx = S.box(case)
            pil_box = None if bx is None else tuple(v / 16 for v in bx)
            differing = 0
            for b in range(S.B):
                img = Image.fromarray(S.frames(h, w)[b].numpy())
                got = np.asarray(img.resize((wo, ho), pil_filter(f), box=pil_box))
                differing += int((got != ref[b]).sum())
            print(f"scale {S.case_id(case)}: {differing} of {ref.size} bytes differ from Pillow")
            assert differing == 0, S.case_id(case)


# Where the scenes' hard edges must drive a pass past both ends of the byte range: the filters with
# negative lobes, whole frame and box, on every pair in which an output pixel can see a hard edge.
# Three pairs cannot, whatever the code does, and are left out for that reason alone: the 1 x 1 frame
# is constant, so every sum is value * sum(k) and stays inside 0..255; at 11:1 and beyond (33 x 65 ->
# 3 x 5, 16 x 4100 -> 3 x 7) an output pixel averages a hundred and more pixels of binary noise, whose
# weighted sum has a standard deviation of some 30 levels around 127: four and more of them away from
# either end, in a few hundred sums.
CLAMPED_PAIRS = [p for p in S.PAIRS if p[:2] != (1, 1) and p not in ((33, 65, 3, 5), (16, 4100, 3, 7))]


@pytest.mark.parametrize("boxed", [False, True], ids=["whole", "box"])
@pytest.mark.parametrize("f", ["bicubic", "lanczos"])
def test_scenes_reach_the_clamp(f, boxed):
    for pair in CLAMPED_PAIRS:
        h, w, ho, wo = pair
        case = (pair, f, boxed)
        horizontal, vertical = Sc.axis_plans(h, w, (ho, wo), f, S.box(case))
        p = S.frames(h, w).numpy()
        lowest, highest = 0, 255
        for plan, axis in ((horizontal, 2), (vertical, 1)):
            if plan is None:
                continue
            sums = scale_pass_sums_ref(p, *plan, axis=axis)
            lowest, highest = min(lowest, int(sums.min())), max(highest, int(sums.max()))
            p = np.clip(sums, 0, 255).astype(np.uint8)
        print(f"scale {S.case_id(case)}: pass sums from {lowest} to {highest}")
        assert lowest < 0 and highest > 255, (S.case_id(case), lowest, highest)
        assert np.array_equal(p, S.reference(case).numpy())


def dense(bounds, k, in_size):
    """int64 ``[out_size, in_size]``: the plan's coefficients at their source positions."""
    K = np.zeros((bounds.shape[0], in_size), np.int64)
    for xx, (first, n) in enumerate(bounds):
        K[xx, first:first + n] = k[xx, :n]
    return K


@pytest.mark.parametrize("case", [c for c in S.CASES if c[0][1] <= 640], ids=S.case_id)
def test_equals_matrix_formulation(case):
    """Two matrix products with the rounding and the clamp between them."""
    (h, w, ho, wo), f, _ = case
    horizontal, vertical = Sc.axis_plans(h, w, (ho, wo), f, S.box(case))
    p = S.frames(h, w).numpy().astype(np.int64)                       # [B, H, W, 3]
    if horizontal is not None:
        Kh = dense(*horizontal, w)                                    # [Wo, W]
        p = np.clip((np.einsum("ow,bhwc->bhoc", Kh, p) + (1 << 21)) >> 22, 0, 255)
    if vertical is not None:
        Kv = dense(*vertical, h)                                      # [Ho, H]
        p = np.clip((np.einsum("oh,bhwc->bowc", Kv, p) + (1 << 21)) >> 22, 0, 255)
    assert np.array_equal(p.astype(np.uint8), S.reference(case).numpy())


def test_plan_properties():
    """Every row sums to 2^22 within n units (n roundings of at most half a unit each, and the
    division's own error far below one), and 255 * sum|k| + 2^21 stays in int32."""
    for case in S.CASES:
        (h, w, ho, wo), f, _ = case
        for plan, in_size in zip(Sc.axis_plans(h, w, (ho, wo), f, S.box(case)), (w, h)):
            if plan is None:
                continue
            bounds, k = plan
            first, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
            assert (first >= 0).all() and (n >= 1).all() and (first + n <= in_size).all() and (n <= k.shape[1]).all()
            assert (np.diff(first) >= 0).all() and (np.diff(first + n) >= 0).all()       # the kernel's window
            k64 = k.astype(np.int64)
            assert (np.abs(k64.sum(1) - (1 << 22)) <= n).all(), S.case_id(case)
            assert (255 * np.abs(k64).sum(1) + (1 << 21) < (1 << 31)).all(), S.case_id(case)
            for xx in range(bounds.shape[0]):
                assert not k[xx, n[xx]:].any()


def test_identity_and_constant():
    f = S.frames(37, 53)
    for name in S.FILTER_NAMES:
        out = scale_frames_ref(f, (37, 53), name)
        assert torch.equal(out, f) and out.data_ptr() != f.data_ptr()
        assert Sc.axis_plans(37, 53, (37, 53), name) == (None, None)
        assert Sc.axis_plans(37, 53, (37, 53), name, (0, 0, 16 * 53, 16 * 37)) == (None, None)
        for size in ((37, 53), (91, 17), (5, 200), (1, 1)):
            for value in (0, 1, 127, 254, 255):
                flat = torch.full((1, 37, 53, 3), value, dtype=torch.uint8)
                for bx in (None, (20, 8, 16 * 53 - 12, 16 * 37 - 24)):
                    assert (scale_frames_ref(flat, size, name, bx) == value).all(), (name, size, value, bx)


def test_box_filter_against_the_redaction_cell_mean():
    """At an integer ratio f the ``box`` filter averages f x f cells as the redaction's pixelate mode
    does, but rounds twice (rows of a cell, then the rounded row means) where the redaction rounds the
    cell's sum once: the two agree only where both roundings fall alike, and differ by one level
    elsewhere."""
    from aiko_services_amd.ops.reference import redact_detections_ref
    h, w, f = 48, 64, 4
    frames = S.frames(h, w)
    det = torch.tensor([[[0.0, 0.0, float(w), float(h), 1.0, 0.0]]]).repeat(S.B, 1, 1)
    count = torch.ones(S.B, dtype=torch.int32)
    cells = redact_detections_ref(frames, det, count, 1, mode="pixelate", block=f)[:, ::f, ::f]
    S_ = frames.to(torch.int64).view(S.B, h // f, f, w // f, f, 3).sum((2, 4))
    assert torch.equal(cells.to(torch.int64), (2 * S_ + f * f) // (2 * f * f))     # the whole frame was covered
    out = scale_frames_ref(frames, (h // f, w // f), "box")
    diff = (out.to(torch.int64) - cells.to(torch.int64)).abs()
    print(f"box at {f}:1 against the cell mean: {int((diff > 0).sum())} of {diff.numel()} bytes differ, by at most "
          f"{int(diff.max())}")
    assert int(diff.max()) <= 1 and int((diff > 0).sum()) > 0


def test_refusals():
    for args, match in [((10, 5, "cubic"), "filter"), ((0, 5, "box"), "sizes"), ((5, 0, "box"), "sizes"),
                        ((Sc.MAX_SIDE + 1, 5, "box"), "sizes"), ((10, 5, "box", -1, 160), "box edges"),
                        ((10, 5, "box", 0, 161), "box edges"), ((10, 5, "box", 80, 80), "box edges"),
                        ((10, 5, "box", 0.5, 160), "integer"), ((10.0, 5, "box"), "integer"),
                        ((4098, 1, "box"), "MAX_TAPS"), ((1366, 2, "lanczos"), "MAX_TAPS")]:
        with pytest.raises(ValueError, match=match):
            Sc.axis_plan(*args)
    assert Sc.MAX_TAPS >= 97
    assert Sc.axis_plan(4096, 1, "box")[1].shape == (1, Sc.MAX_TAPS)           # the limit itself is served
    assert Sc.axis_plan(1552, 16, "lanczos")[1].shape == (16, 583)
    for args, kw, match in [((10, 10, (5, 5), "nearest"), {}, "filter"), ((10, 10, (0, 5)), {}, "sizes"),
                            ((10, 10, (5,)), {}, "size ="), ((10, 10, 5), {}, "size ="),
                            ((10, 10, (5, 5)), dict(box=(0, 0, 161, 160)), "outside the frame"),
                            ((10, 10, (5, 5)), dict(box=(0, 0, 160)), "box ="),
                            ((10, 10, (5, 5)), dict(box=(16, 0, 16, 160)), "outside the frame"),
                            ((10, 10, (5, 5)), dict(box=(0, 0, 160.0, 160)), "integer"),
                            ((5000, 10, (1, 5), "box"), {}, "MAX_TAPS")]:
        with pytest.raises(ValueError, match=match):
            Sc.scale_plan(*args, device="cpu", **kw)
    for bx, match in [((0, 0, 1.03, 2), "1/16"), ((0, 0, 1), "four numbers"), ("abcd", "four numbers"),
                      ((0, 0, float("nan"), 1), "four numbers")]:
        with pytest.raises(ValueError, match=match):
            Sc.box_from_pixels(bx)
    assert Sc.box_from_pixels([1.25, 0.5, 39.25, 28.5]) == (20, 8, 628, 456)


def test_scale_plan_is_cached_and_tiles_fit():
    a = Sc.scale_plan(97, 131, (70, 150), "bicubic", device="cpu")
    b = Sc.scale_plan(97, 131, [70, 150], "bicubic", None, "cpu")
    assert a is b and a.hk.dtype == torch.int32 and a.vb.shape == (70, 2) and a.size == (70, 150)
    assert a.tile_rows * 1 < 70 and a.tile_cols < 150                          # several tiles in both directions
    one = Sc.scale_plan(64, 64, (64, 31), "bicubic", device="cpu")
    assert one.vb is None and one.vk is None and one.hb.shape == (31, 2)
    for h, ho, f in ((97, 70, "bicubic"), (480, 224, "lanczos"), (4096, 1, "box"), (1552, 16, "lanczos"), (5, 40, "box")):
        bounds, _ = Sc.axis_plan(h, ho, f)
        rows, cols, win = Sc.tile_for(bounds)
        assert 1 <= rows <= Sc.TILE_ROWS and cols in Sc.TILE_COLS and win == Sc.window_rows(bounds, rows)
        assert win * cols * 3 <= Sc.MAX_LDS
        for y0 in range(0, ho, rows):                                          # every tile's rows lie in its window
            y1 = min(y0 + rows, ho)
            assert (bounds[y0:y1, 0] >= bounds[y0, 0]).all()
            assert (bounds[y0:y1, 0] + bounds[y0:y1, 1] <= bounds[y0, 0] + win).all()
    assert Sc.tile_for(Sc.axis_plan(4096, 1, "box")[0]) == (1, 12, 4096)       # MAX_TAPS rows: 147456 bytes of LDS


# ---- ImageResize on the host ----------------------------------------------------------------

def image_resize(**parameters):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    d = {"version": 0, "name": "p_resize", "runtime": "python", "graph": ["(ImageResize)"], "parameters": {},
         "elements": [{"name": "ImageResize", "input": [{"name": "images", "type": "[image]"}],
                       "output": [{"name": "images", "type": "[image]"}], "parameters": parameters,
                       "deploy": {"local": {"module": "aiko_services_amd.elements.media.image_io"}}}]}
    p = PipelineImpl.create_pipeline("<resize>", parse_pipeline_definition_dict(d), None, None, "c", [], 0, None, 60,
                                     queue_response=queue.Queue())
    return p.pipeline_graph.get_node("ImageResize").element


def test_image_resize_host_branch():
    Image = pytest.importorskip("PIL.Image")
    from aiko_services_amd.pipeline.stream import StreamEvent
    frames = S.frames(37, 53)
    images = [f.numpy() for f in frames]
    for name in S.FILTER_NAMES:
        event, out = image_resize(resolution="17x91", filter=name).process_frame(None, images)
        assert event == StreamEvent.OKAY
        assert np.array_equal(np.stack(out["images"]), scale_frames_ref(frames, (91, 17), name).numpy()), name
    # without ``filter``: what it returned before, bilinear through Pillow; PIL images stay PIL images
    element = image_resize(resolution="17x91")
    event, out = element.process_frame(None, images)
    assert event == StreamEvent.OKAY
    for got, image in zip(out["images"], images):
        assert np.array_equal(got, np.asarray(Image.fromarray(image).resize((17, 91), Image.BILINEAR)))
    event, out = element.process_frame(None, [Image.fromarray(images[0])])
    assert isinstance(out["images"][0], Image.Image) and out["images"][0].size == (17, 91)
    event, out = image_resize(resolution="17x91", filter="nearest").process_frame(None, images)
    assert event == StreamEvent.ERROR and "filter" in out["diagnostic"]
