"""Scenes of the motion-detection tests (``ops/motion.py``), shared by test_motion_reference.py
(what ``motion_detect_ref`` must give, and what the scenes must cover) and test_gpu_motion.py (the
kernels against ``motion_detect_ref``, step by step).  A scene's reference run is computed once per
process and handed out unchanged.

Three cameras of 45 x 150 (150: the byte path; 152, a multiple of 4: the dword path): two tiles
across and two tile rows of the kernel's 128 x 32 tile, partial cells right and bottom at every
cell size.  Seven frames; camera 2 starts from a garbage state with ``seen < 0``.

A plain module (no fixtures, no device requirement), like kernel_guard.py."""
from __future__ import annotations

import functools

import torch

B, H, W = 3, 45, 150
W4 = 152
WIDTHS = (W, W4)
CELLS = (8, 16, 32)
TILE_W, TILE_H = 128, 32       # pixels per workgroup of motion_cells_kernel (MO_TW, MO_TH)
LO = (40, 40, 40)              # luma 40
HI = (200, 90, 30)             # luma (77*200 + 150*90 + 29*30 + 128) >> 8 = 116
THRESHOLD = 12
BASE = dict(threshold=THRESHOLD, learn_shift=4, learn_moving=True, warmup=1, min_cells=2, max_det=2)
VARIANTS = {"base": {}, "warmup3": {"warmup": 3}, "frozen": {"learn_moving": False}}
FRAMES = 7


def grid(cell, width=W, height=H):
    return -(-height // cell), -(-width // cell)


def frame_from_mask(moving, cell, width=W, height=H, lo=LO, hi=HI):
    """uint8 ``[height, width, 3]``: the pixels of the cells ``moving`` {(gy, gx), ...} at ``hi``, the
    rest at ``lo``."""
    f = torch.empty(height, width, 3, dtype=torch.uint8)
    f[:] = torch.tensor(lo, dtype=torch.uint8)
    for gy, gx in moving:
        f[gy * cell:(gy + 1) * cell, gx * cell:(gx + 1) * cell] = torch.tensor(hi, dtype=torch.uint8)
    return f


def raise_pixels(f, gy, gx, cell, share):
    """One luma level more on the first ``share`` (a fraction) of the pixels of the FULL cell (gy, gx)
    of a grey frame: its level rises by ``16 * share`` sixteenths (rounded half down: 1/16 -> 1,
    1/2 -> 8)."""
    n = int(cell * cell * share)
    block = f[gy * cell:(gy + 1) * cell, gx * cell:(gx + 1) * cell]
    assert block.shape[:2] == (cell, cell)
    flat = block.reshape(-1, 3).clone()
    flat[:n] += 1
    f[gy * cell:(gy + 1) * cell, gx * cell:(gx + 1) * cell] = flat.view(cell, cell, 3)


def patterns(cell, width=W):
    """The cell sets the scripted frames are made of."""
    gh, gw = grid(cell, width)
    bx = TILE_W // cell                                     # the first cell column of the second tile
    return {
        "pairs": {(y, x) for x in (0, 2, 4) for y in (0, 1)},           # three components of area 2
        "single_and_diagonal": {(0, 0), (0, 2), (1, 3)},                # area 1; two cells joined by a corner
        "crossing": {(0, bx - 1), (0, bx)},                             # over the tile boundary at x = 128
        "crossing_and_corner": {(0, bx - 1), (0, bx), (gh - 1, gw - 1), (gh - 1, gw - 2)},
    }


def edge_frame(cell, width=W):
    """Camera 2's scripted frame over a background of exactly 16 * 40: cell (0, 0) differs by exactly
    16 * THRESHOLD sixteenths, (0, 1) by one more, (0, 2) by -16 and (0, 3) by +8."""
    f = frame_from_mask((), cell, width)
    up = tuple(c + THRESHOLD for c in LO)
    for gx in (0, 1):
        f[0:cell, gx * cell:(gx + 1) * cell] = torch.tensor(up, dtype=torch.uint8)
    raise_pixels(f, 0, 1, cell, 1 / 16)
    f[0:cell, 2 * cell:3 * cell] = torch.tensor(tuple(c - 1 for c in LO), dtype=torch.uint8)
    raise_pixels(f, 0, 3, cell, 1 / 2)
    return f


class Scene:
    """``frames`` [uint8 [B, H, width, 3], ...] stepped from ``state0`` with the parameters ``kw``."""

    def __init__(self, cell, width, variant):
        from aiko_services_amd.ops.motion import MotionState, new_state
        self.cell, self.width, self.variant = cell, width, variant
        self.kw = {**BASE, **VARIANTS[variant], "cell": cell}
        p = patterns(cell, width)
        still = ()
        g = torch.Generator().manual_seed(1000 + cell + width)
        noise = lambda: torch.randint(0, 256, (H, width, 3), dtype=torch.uint8, generator=g)  # noqa: E731
        fm = lambda cells: frame_from_mask(cells, cell, width)  # noqa: E731
        per_camera = [
            [still, p["pairs"], p["single_and_diagonal"], p["pairs"], p["single_and_diagonal"], still, p["crossing"]],
            [still, p["crossing"], still, p["crossing_and_corner"], still, p["pairs"], p["single_and_diagonal"]],
        ]
        cam2 = [fm(still), fm(still), edge_frame(cell, width), fm(still), noise(), noise(), noise()]
        self.frames = [torch.stack([fm(per_camera[0][t]), fm(per_camera[1][t]), cam2[t]]) for t in range(FRAMES)]
        # camera 2: garbage, and a negative frame count: the first frame must simply become its background
        state = new_state(B, H, width, cell, "cpu")
        state.bg[2] = torch.randint(-2 ** 31, 2 ** 31 - 1, state.bg[2].shape, generator=g).to(torch.int32)
        state.seen[2] = -7
        self.state0 = MotionState(state.bg, state.seen)


@functools.lru_cache(maxsize=None)
def scene(cell, width=W, variant="base"):
    return Scene(cell, width, variant)


@functools.lru_cache(maxsize=None)
def reference(cell, width=W, variant="base"):
    """``((det, count, mask, cells, state_out), ...)`` of ``motion_detect_ref``, one per frame;
    computed once, not to be modified."""
    from aiko_services_amd.ops.reference import motion_detect_ref
    s = scene(cell, width, variant)
    state, steps = s.state0, []
    for f in s.frames:
        out = motion_detect_ref(f, state, **s.kw)
        state = out[4]
        steps.append(out)
    return tuple(steps)


def levels(frames, cell):
    """``cur`` of every cell, int32 ``[B, Gh, Gw]``: the background an empty state takes from ``frames``."""
    from aiko_services_amd.ops.motion import new_state
    from aiko_services_amd.ops.reference import motion_detect_ref
    b, h, w, _ = frames.shape
    return motion_detect_ref(frames, new_state(b, h, w, cell, "cpu"), cell=cell)[4].bg


def components(mask):
    """{label: (area, cx0, cy0, cx1, cy1)} of a uint8 ``[Gh, Gw]`` mask by a depth-first walk."""
    gh, gw = mask.shape
    seen, out = set(), {}
    for gy in range(gh):
        for gx in range(gw):
            if not mask[gy, gx] or (gy, gx) in seen:
                continue
            stack, cells = [(gy, gx)], []
            seen.add((gy, gx))
            while stack:
                y, x = stack.pop()
                cells.append((y, x))
                for ny in range(max(y - 1, 0), min(y + 2, gh)):
                    for nx in range(max(x - 1, 0), min(x + 2, gw)):
                        if mask[ny, nx] and (ny, nx) not in seen:
                            seen.add((ny, nx))
                            stack.append((ny, nx))
            ys, xs = [c[0] for c in cells], [c[1] for c in cells]
            out[gy * gw + gx] = (len(cells), min(xs), min(ys), max(xs), max(ys))
    return out


def assert_conditions(cell, width=W):
    """What the scenes must exercise, asserted on the reference's own results, so that a scene cannot
    quietly stop exercising a rule."""
    s, ref = scene(cell, width), reference(cell, width)
    kw = s.kw
    gh, gw = grid(cell, width)
    assert len(s.frames) >= 6 and gh * cell > H                             # state carries; partial cells below
    assert gw * cell > width or (width, cell) == (W4, 8)                    # ... and right (152 = 19 * 8)
    assert gw * cell > TILE_W and gh * cell > TILE_H                        # more than one tile each way
    comps = [[components(step[2][b]) for b in range(B)] for step in ref]
    qualifying = lambda c: [k for k, v in c.items() if v[0] >= kw["min_cells"]]  # noqa: E731
    # more qualifying components than max_det, two of them of equal area: the tie rule decides
    t, b = 1, 0
    q = qualifying(comps[t][b])
    assert len(q) > kw["max_det"] and int(ref[t][1][b]) == kw["max_det"]
    assert len({comps[t][b][k][0] for k in q}) == 1
    assert [float(x) for x in ref[t][0][b, :, 0]] == [0.0, 2.0 * cell]      # the two lowest labels, in order
    # a component dropped by min_cells, and two cells joined only by a corner
    t, b = 2, 0
    assert any(v[0] < kw["min_cells"] for v in comps[t][b].values())
    assert int(ref[t][3][b]) == 3 and int(ref[t][1][b]) == 1
    area, cx0, cy0, cx1, cy1 = comps[t][b][2]
    assert (area, cx1 - cx0, cy1 - cy0) == (2, 1, 1) and float(ref[t][0][b, 0, 4]) == 0.5
    # a component over the 128-pixel tile boundary
    t, b = 1, 1
    x1, _, x2, _ = (float(v) for v in ref[t][0][b, 0, :4])
    assert int(ref[t][1][b]) == 1 and x1 < TILE_W < x2
    # exactly 16 * threshold does not move, one sixteenth more does; half-up rounding and the floor
    # of a negative difference both change the background
    t, b = 2, 2
    cur, bg, new = levels(s.frames[t], cell)[b], ref[t - 1][4].bg[b], ref[t][4].bg[b]
    d = (cur.long() - bg.long())[0]
    assert d[:4].tolist() == [16 * THRESHOLD, 16 * THRESHOLD + 1, -16, 8]
    assert ref[t][2][b, 0, :4].tolist() == [0, 1, 0, 0]
    step = (new.long() - bg.long())[0, :4].tolist()
    shift, half = kw["learn_shift"], 1 << (kw["learn_shift"] - 1)
    assert step[2] == -1 and int((-16 + half) / 2 ** shift) == 0            # floor, not truncation
    assert step[3] == 1 and 8 >> shift == 0                                 # half up, not floor alone
    # seen < 0 over garbage: the frame becomes the background, nothing moves
    first = ref[0]
    assert int(s.state0.seen[2]) < 0 and int(first[4].seen[2]) == 1 and int(first[3][2]) == 0
    assert torch.equal(first[4].bg[2], levels(s.frames[0], cell)[2])
    assert [int(x) for x in ref[-1][4].seen] == [FRAMES] * B
    # the noise frames: every cell moves, one component
    assert int(ref[4][3][2]) == gh * gw and int(ref[4][1][2]) == 1
    # warmup 3: nothing is reported while s < 3, although the base scene reports there
    warm = reference(cell, width, "warmup3")
    assert all(int(warm[t][3].sum()) == 0 for t in range(3)) and int(ref[1][3].sum()) > 0
    assert int(warm[3][3].sum()) > 0
    # learn_moving false keeps the background of a moving cell
    frozen = reference(cell, width, "frozen")
    assert not torch.equal(frozen[-1][4].bg, ref[-1][4].bg)
    assert int(frozen[1][4].bg[0, 0, 0]) == 16 * 40 != int(ref[1][4].bg[0, 0, 0])


# ---- labelling worst cases: cell masks on the full 128 x 128 grid (cell 8, 1024 x 1024) ------------

WORST_CELL, WORST_SIDE = 8, 1024


def worst_masks():
    """{name: bool [128, 128]}: what the labelling rounds find hardest, and the two trivial ends."""
    n = WORST_SIDE // WORST_CELL
    serp = torch.zeros(n, n, dtype=torch.bool)
    serp[0::2, :] = True                                    # every other row, joined at alternating ends
    for i, gy in enumerate(range(1, n, 2)):
        serp[gy, n - 1 if i % 2 == 0 else 0] = True
    yy, xx = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    return {"serpentine": serp, "serpentine_t": serp.t().contiguous(), "checkerboard": (yy + xx) % 2 == 0,
            "all": torch.ones(n, n, dtype=torch.bool), "empty": torch.zeros(n, n, dtype=torch.bool)}


def worst_case(mask):
    """(frame uint8 ``[1, 1024, 1024, 3]`` with ``mask``'s cells at ``HI`` over ``LO``, the state of a
    camera that has seen one still ``LO`` frame)."""
    from aiko_services_amd.ops.motion import MotionState
    n = WORST_SIDE // WORST_CELL
    frame = frame_from_mask((), WORST_CELL, WORST_SIDE, WORST_SIDE).view(n, WORST_CELL, n, WORST_CELL, 3)
    gy, gx = mask.nonzero(as_tuple=True)
    frame[gy, :, gx] = torch.tensor(HI, dtype=torch.uint8)
    state = MotionState(torch.full((1, n, n), 16 * LO[0], dtype=torch.int32), torch.ones(1, dtype=torch.int32))
    return frame.view(1, WORST_SIDE, WORST_SIDE, 3), state
