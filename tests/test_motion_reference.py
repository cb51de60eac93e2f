"""``ops.reference.motion_detect_ref`` — the definition the motion kernels are held to
(test_gpu_motion.py) — against the rule of ops/motion.py, and the scenes of motion_scenes.py against
what they claim to exercise.  CPU only."""
import numpy as np
import pytest
import torch

import motion_scenes as S
from motion_scenes import B, H

CONFIGS = [(cell, width) for cell in S.CELLS for width in S.WIDTHS]


@pytest.mark.parametrize("cell,width", CONFIGS)
def test_scenes_exercise_every_rule(cell, width):
    S.assert_conditions(cell, width)


@pytest.mark.parametrize("cell,width", CONFIGS)
def test_rows_are_exactly_their_cells_pixels(cell, width):
    from aiko_services_amd.ops.reference import roi_rects_ref
    kw = S.scene(cell, width, "base").kw
    rows = 0
    for det, count, mask, cells, _ in S.reference(cell, width, "base"):
        rects = roi_rects_ref(det, count, kw["max_det"], (H, width), 0.0).view(B, kw["max_det"], 4)
        for b in range(B):
            comps = S.components(mask[b])
            assert int(cells[b]) == sum(v[0] for v in comps.values()) == int(mask[b].sum())
            best = sorted((k for k, v in comps.items() if v[0] >= kw["min_cells"]),
                          key=lambda k: (-comps[k][0], k))[:kw["max_det"]]
            assert int(count[b]) == len(best)
            for i, k in enumerate(best):
                area, cx0, cy0, cx1, cy1 = comps[k]
                want = [cx0 * cell, cy0 * cell, min((cx1 + 1) * cell, width), min((cy1 + 1) * cell, H)]
                assert rects[b, i].tolist() == want and det[b, i, :4].tolist() == [float(v) for v in want]
                assert float(det[b, i, 4]) == float(np.float32(area / ((cx1 - cx0 + 1) * (cy1 - cy0 + 1))))
                assert float(det[b, i, 5]) == 0.0
                rows += 1
            assert not det[b, len(best):].any() and not rects[b, len(best):].any()
    assert rows > 10


@pytest.mark.parametrize("variant", sorted(S.VARIANTS))
def test_state_carries_and_cameras_are_independent(variant):
    from aiko_services_amd.ops.motion import MotionState
    from aiko_services_amd.ops.reference import motion_detect_ref
    cell, width = 16, S.W
    s, ref = S.scene(cell, width, variant), S.reference(cell, width, variant)
    # resumed at frame 3 from a copy of the carried state: the same steps
    state = MotionState(*(t.clone() for t in ref[2][4]))
    for t in range(3, S.FRAMES):
        out = motion_detect_ref(s.frames[t], state, **s.kw)
        for got, want in zip((*out[:4], *out[4]), (*ref[t][:4], *ref[t][4])):
            assert got.dtype == want.dtype and torch.equal(got, want)
        state = out[4]
    # one camera alone: its rows of the batch
    for b in range(B):
        state = MotionState(s.state0.bg[b:b + 1], s.state0.seen[b:b + 1])
        for t in range(S.FRAMES):
            out = motion_detect_ref(s.frames[t][b:b + 1], state, **s.kw)
            for got, want in zip((*out[:4], *out[4]), (*ref[t][:4], *ref[t][4])):
                assert torch.equal(got, want[b:b + 1])
            state = out[4]
    # the state handed in is not modified
    assert int(s.state0.seen[2]) == -7


def test_empty_state_grid_and_parameters():
    from aiko_services_amd.ops import motion as M
    state = M.new_state(2, 45, 150, 16, "cpu")
    assert isinstance(state, M.MotionState) and state.bg.shape == (2, 3, 10) and state.seen.shape == (2,)
    assert state.bg.dtype == state.seen.dtype == torch.int32 and not state.bg.any() and not state.seen.any()
    assert M.CELLS == (8, 16, 32)
    assert M.grid_shape(1080, 1920, 16) == (68, 120) and M.grid_shape(480, 640, 8) == (60, 80)
    assert M.grid_shape(1, 1, 32) == (1, 1) and M.grid_shape(33, 32, 32) == (2, 1)
    for cell in (0, 4, 12, 64, True):
        with pytest.raises(ValueError, match="cell"):
            M.grid_shape(45, 150, cell)
    ok = dict(cell=16, threshold=12, learn_shift=4, warmup=1, min_cells=2, max_det=16)
    M.check_parameters(**ok)
    M.check_parameters(**{**ok, "threshold": 0, "learn_shift": 0, "max_det": 64})
    M.check_parameters(**{**ok, "threshold": 255, "learn_shift": 8, "max_det": 1})
    for name, bad in (("cell", 4), ("threshold", -1), ("threshold", 256), ("threshold", 1.5), ("learn_shift", -1),
                      ("learn_shift", 9), ("warmup", 0), ("min_cells", 0), ("max_det", 0), ("max_det", 65)):
        with pytest.raises(ValueError, match=name):
            M.check_parameters(**{**ok, name: bad})


def test_luma_of_every_rgb_triple_is_a_byte():
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    lo, hi = 255, 0
    for r in range(256):
        y = (77 * r + 150 * g + 29 * b + 128) >> 8
        lo, hi = min(lo, int(y.min())), max(hi, int(y.max()))
    assert (lo, hi) == (0, 255)


@pytest.mark.parametrize("cell", S.CELLS)
def test_levels_of_uniform_frames(cell):
    from aiko_services_amd.ops.motion import new_state
    from aiko_services_amd.ops.reference import motion_detect_ref
    for value in (0, 1, 40, 255):
        frames = torch.full((1, 45, 150, 3), value, dtype=torch.uint8)
        out = motion_detect_ref(frames, new_state(1, 45, 150, cell, "cpu"), cell=cell)
        assert bool((out[4].bg == 16 * value).all()) and 16 * 255 == 4080      # partial cells too
        assert int(out[1][0]) == 0 and int(out[3][0]) == 0 and not out[2].any()


def test_background_stalls_half_a_level_short():
    """From 0 towards 3200 at shift 4 the background ends at 3193 (ops/motion.py, rule 5)."""
    from aiko_services_amd.ops.motion import MotionState
    from aiko_services_amd.ops.reference import motion_detect_ref
    frames = torch.full((1, 8, 8, 3), 200, dtype=torch.uint8)
    state = MotionState(torch.zeros(1, 1, 1, dtype=torch.int32), torch.ones(1, dtype=torch.int32))
    for _ in range(200):
        state = motion_detect_ref(frames, state, cell=8, learn_shift=4)[4]
    assert int(state.bg[0, 0, 0]) == 3193 and int(state.seen[0]) == 201


def test_worst_case_masks_are_what_they_claim():
    masks = S.worst_masks()
    n = S.WORST_SIDE // S.WORST_CELL
    assert n * n == 16384
    for name in ("serpentine", "serpentine_t", "checkerboard", "all"):
        comps = S.components(masks[name].to(torch.uint8))
        assert len(comps) == 1 and comps[0][0] == int(masks[name].sum()), name
    assert int(masks["serpentine"].sum()) == 64 * 128 + 64 and not masks["empty"].any()
    frame, state = S.worst_case(masks["serpentine"])
    assert torch.equal(S.levels(frame, S.WORST_CELL)[0] > 16 * 40, masks["serpentine"]) and int(state.seen[0]) == 1
