"""``warp_quads_ref`` (``ops/reference.py``), the numpy float64 form of the rule of ``ops/warp.py``, on
the CPU: the six named views are exact pixel permutations, every marker the marker reference finds
reads back its own module grid from its rectified patch, step 2 stays below 2^53, the slot rules,
the vectorised form against plain loops, and the front end's refusals."""
import itertools

import numpy as np
import pytest
import torch

import marker_scenes as S
import warp_scenes as WS
from aiko_services_amd.ops.reference import warp_coefficients_ref, warp_quads_ref
from aiko_services_amd.ops.warp import VIEWS, check_parameters, view_quad, warp_quads


@pytest.mark.parametrize("h,w", WS.VIEW_SIZES)
@pytest.mark.parametrize("name", VIEWS)
def test_named_views_are_exact_permutations(name, h, w):
    frames = WS.noise(h, w, b=2)
    quads, count, size = WS.view_case(name, h, w, b=2)
    patches, valid = warp_quads_ref(frames, quads, count, 1, size, 0, "edge")
    want = WS.numpy_view(name, frames)
    assert size == ((w, h) if name in ("rot90", "rot270") else (h, w)) and tuple(patches.shape) == (2, *size, 3)
    assert valid.tolist() == [1, 1] and patches.dtype == torch.uint8
    assert torch.equal(patches, want), name


@pytest.mark.parametrize("margin,side", WS.SETTINGS)
def test_every_marker_reads_back_its_module_grid(margin, side):
    found = 0
    for name in WS.MARKER_SCENES:
        frames, corners, count, ids = WS.marker_case(name)
        patches, valid = WS.reference(name, S.W, 16, (side, side), margin)
        for b in range(S.B):
            n = int(count[b])
            assert valid[b * 16:(b + 1) * 16].tolist() == [1] * n + [0] * (16 - n)
            assert not patches[b * 16 + n:(b + 1) * 16].any()
            for i in range(n):
                got = WS.read_modules(patches[b * 16 + i], 7, margin)
                assert np.array_equal(got, S.module_grid("original", int(ids[b, i]))), (name, b, i, margin, side)
                found += 1
    assert found == 33


def test_step_2_stays_below_2_to_the_53():
    worst = 0
    for origin in ("centre", "edge"):
        for corner in itertools.product((-4096, 8191), repeat=8):
            c = warp_coefficients_ref(list(zip(corner[0::2], corner[1::2])), origin)
            if c is not None:
                worst = max(worst, max(abs(x) for x in c))
                assert c[2] > 0
    assert 2 ** 40 < worst < 2 ** 53, worst
    # and wherever the corners lie in the range: a difference is at most d, a doubled coordinate at most
    # x, so |den| <= 2 d^2, |G|, |Hh| <= 4 d^2 and the largest, |A|, at most 2 d^3 + 4 d^2 x
    d, x = 2 * (8191 + 4096), 2 * 8192
    assert worst <= 2 * d ** 3 + 4 * d ** 2 * x < 2 ** 53
    # the largest used quad samples the frame like any other
    frames = WS.noise(9, 12)
    quads = torch.tensor(WS.EXTREME, dtype=torch.int32).view(1, 1, 4, 2)
    patches, valid = warp_quads_ref(frames, quads, torch.ones(1, dtype=torch.int32), 1, (8, 8))
    assert valid.tolist() == [1]
    assert torch.equal(patches[0, 0, 0], frames[0, 0, 0]) and torch.equal(patches[0, 7, 7], frames[0, 8, 11])


def _slots(quads, count, k, frames=None, **kw):
    frames = WS.noise(40, 48).clamp(min=1) if frames is None else frames
    q = torch.tensor(quads, dtype=torch.int32).view(1, -1, 4, 2)
    return warp_quads_ref(frames, q, torch.tensor([count], dtype=torch.int32), k, kw.pop("size", (8, 8)), **kw)


def test_slot_rules():
    good = [(4, 4), (30, 6), (28, 30), (6, 26)]
    # count above k is capped at k; a negative count is zero
    patches, valid = _slots([good] * 4, 9, 3)
    assert valid.tolist() == [1, 1, 1] and patches.shape[0] == 3 and all(p.all() for p in patches)
    for count in (-1, -2 ** 31, 0):
        patches, valid = _slots([good] * 4, count, 3)
        assert valid.tolist() == [0, 0, 0] and not patches.any()
    # unused kinds among used slots: zeros and valid 0 there, the others as alone
    alone, _ = _slots([good], 1, 1)
    for kind, quad in WS.UNUSED.items():
        patches, valid = _slots([good, quad, good], 3, 3)
        assert valid.tolist() == [1, 0, 1] and not patches[1].any(), kind
        assert torch.equal(patches[0], alone[0]) and torch.equal(patches[2], alone[0]), kind
    # the limits themselves are used
    patches, valid = _slots([[(8191, 4), (30, 6), (28, 30), (6, 26)], [(4, -4096), (30, 6), (28, 30), (6, 26)]], 2, 2)
    assert valid.tolist() == [1, 1]


def test_margin_across_the_horizon_is_zero_where_w_is_not_positive():
    G, Hh, den = (np.float64(x) for x in warp_coefficients_ref(WS.HORIZON)[:3])
    ho, wo, m = 40, 48, 64
    u = ((2 * np.arange(wo) + 1) * (8 + m) - m * wo) / np.float64(16 * wo)
    v = (((2 * np.arange(ho) + 1) * (8 + m) - m * ho) / np.float64(16 * ho))[:, None]
    behind = torch.from_numpy(~(((G * u) + (Hh * v)) + den > 0))
    assert behind.any() and not behind.all()
    patches, valid = _slots([WS.HORIZON], 1, 1, frames=WS.noise(176, 208).clamp(min=1), size=(ho, wo), margin=m)
    assert valid.tolist() == [1]
    assert torch.equal((patches[0] == 0).all(-1), behind)           # the frame has no zero byte


def test_clamp_at_all_four_frame_edges():
    """The whole frame with a margin of one side all round, at three times the size: the frame in the
    middle, its edge pixels repeated around it."""
    h, w = 9, 12
    frames = WS.noise(h, w)
    quads, count, size = WS.view_case("identity", h, w)
    patches, _ = warp_quads_ref(frames, quads, count, 1, (3 * h, 3 * w), 16, "edge")
    want = np.pad(frames[0].numpy(), ((h, h), (w, w), (0, 0)), mode="edge")
    assert torch.equal(patches[0], torch.from_numpy(want))
    # and a marker-style quad (pixel centres) over each corner of the frame
    for quad in ([(-5, -4), (6, -3), (5, 5), (-4, 4)], [(8, 5), (16, 4), (17, 12), (7, 11)]):
        q = torch.tensor(quad, dtype=torch.int32).view(1, 1, 4, 2)
        patches, valid = warp_quads_ref(frames, q, count, 1, (16, 16), 3)
        assert valid.tolist() == [1]
        assert torch.equal(patches[0], torch.tensor(WS.warp_pixel_loops(frames[0].tolist(), quad, (16, 16), 3, "centre"),
                                                    dtype=torch.uint8))


@pytest.mark.parametrize("origin", ("centre", "edge"))
@pytest.mark.parametrize("margin", (0, 5, 64))
def test_vectorised_equals_plain_loops(margin, origin):
    h, w, size = 20, 27, (10, 14)
    frames = WS.noise(h, w, seed=margin)
    rng = np.random.default_rng(margin)
    quads = [WS.convex_quad(rng, h, w, spill=6) for _ in range(4)] + [WS.UNUSED["collinear"], WS.HORIZON]
    q = torch.tensor(quads, dtype=torch.int32).view(1, -1, 4, 2)
    patches, valid = warp_quads_ref(frames, q, torch.tensor([6], dtype=torch.int32), 6, size, margin, origin)
    for i, quad in enumerate(quads):
        want = WS.warp_pixel_loops(frames[0].tolist(), quad, size, margin, origin)
        assert int(valid[i]) == (want is not None)
        want = torch.zeros(*size, 3, dtype=torch.uint8) if want is None else torch.tensor(want, dtype=torch.uint8)
        assert torch.equal(patches[i], want), (i, quad)


def test_front_end_refusals():
    check_parameters(4, (224, 224), 0, "centre")
    check_parameters(1, (1, 4), 64, "edge")
    check_parameters(np.int64(4), [4096, 4096], np.int32(3), "edge")
    for bad, match in ((dict(k=0), "k an integer"), (dict(k=True), "k an integer"), (dict(k=2.0), "k an integer"),
                       (dict(size=(224,)), "size"), (dict(size=224), "size"), (dict(size=(8.0, 8)), "size"),
                       (dict(size=(0, 8)), "Ho, Wo"), (dict(size=(8, 4100)), "Ho, Wo"), (dict(size=(4097, 8)), "Ho, Wo"),
                       (dict(size=(8, 6)), "multiple of 4"), (dict(margin=-1), "margin"), (dict(margin=65), "margin"),
                       (dict(margin=0.5), "margin"), (dict(margin=False), "margin"), (dict(origin="corner"), "origin"),
                       (dict(origin=None), "origin")):
        with pytest.raises(ValueError, match=match):
            check_parameters(**{**dict(k=4, size=(224, 224), margin=0, origin="centre"), **bad})
    # warp_quads checks before it reaches the operator
    frames, quads, count = WS.noise(8, 8), torch.zeros(1, 1, 4, 2, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="multiple of 4"):
        warp_quads(frames, quads, count, k=1, size=(8, 10))
    with pytest.raises(ValueError, match="frames"):
        warp_quads(frames[0], quads, count, k=1, size=(8, 8))
    with pytest.raises(ValueError, match="patches"):
        warp_quads(frames, quads, count, k=1, size=(8, 8), patches=torch.empty(1, 8, 12, 3, dtype=torch.uint8))
    # the reference takes any width, and refuses what the rule refuses
    with pytest.raises(ValueError, match="margin"):
        warp_quads_ref(frames, quads, count, 1, (8, 8), 65)
    with pytest.raises(ValueError, match="quads"):
        warp_quads_ref(frames, quads, count, 2, (8, 8))
    # view_quad
    assert view_quad("identity", 3, 5) == ([(0, 0), (5, 0), (5, 3), (0, 3)], (3, 5))
    assert view_quad("rot90", 3, 5)[1] == (5, 3) and view_quad("rot270", 3, 5)[1] == (5, 3)
    for name in VIEWS:
        quad, size = view_quad(name, 3, 5)
        assert sorted(quad) == [(0, 0), (0, 3), (5, 0), (5, 3)]
    for bad, match in ((("transpose", 3, 5), "view one of"), (("rot90", 0, 5), "H, W"), (("rot90", 3, 4097), "H, W"),
                       (("identity", 3.5, 5), "H, W")):
        with pytest.raises(ValueError, match=match):
            view_quad(*bad)
