"""Scenes of the tracker tests (``ops/track.py``): the scripted cases, one per rule, and the seeded
random walk, shared by test_track_reference.py (what ``track_ref`` must give) and
test_gpu_track.py (the kernel against ``track_ref``, step by step).  A scene's reference run is
computed once per process and handed out unchanged.

A plain module (no fixtures, no device requirement), like kernel_guard.py."""
from __future__ import annotations

import functools
import random

import torch

B, MAX_DET, K, T = 3, 6, 4, 5
NAN = float("nan")


def row(x1, y1, x2, y2, score=0.9, cls=0):
    return [float(x1), float(y1), float(x2), float(y2), float(score), float(cls)]


def frame(rows_by_b, counts=None, batch=B, max_det=MAX_DET):
    """(det fp32 [batch, max_det, 6], count int32 [batch]): ``rows_by_b`` {b: [row, ...]}, the count
    of a frame the number of its rows unless ``counts`` {b: count} says otherwise; rows not given
    are zeros."""
    det = torch.zeros(batch, max_det, 6, dtype=torch.float32)
    count = torch.zeros(batch, dtype=torch.int32)
    for b, rows in rows_by_b.items():
        for i, r in enumerate(rows):
            det[b, i] = torch.tensor(row(*r), dtype=torch.float32)
        count[b] = len(rows)
    for b, c in (counts or {}).items():
        count[b] = c
    return det, count


class Scene:
    """Frames ``[(det, count), ...]`` stepped from the empty state with the parameters ``kw``."""

    def __init__(self, frames, k=K, tracks=T, **kw):
        self.frames, self.k, self.tracks, self.kw = list(frames), k, tracks, kw
        self.batch = self.frames[0][0].shape[0]


def _grid(n, x0=0, cls=0):                                  # n disjoint 8 x 8 boxes in a row
    return [(x0 + 10 * i, 0, x0 + 10 * i + 8, 8, 0.9, cls) for i in range(n)]


# every scripted case keeps row 2 at count 0 over garbage: its state must stay all zeros
def _scripted():
    junk = {2: [(5, 5, 9, 9)] * MAX_DET}
    z = {2: 0}

    def f(rows_by_b, counts=None):
        return frame({**junk, **rows_by_b}, {**z, **(counts or {})})

    s = {}
    # inter 3, union 10: fp32(0.3) * 10 > 3 in fp64 (no match), but rounds to 3.0 in fp32
    s["threshold_fp64"] = Scene([f({0: [(0, 0, 5, 1)]}), f({0: [(2, 0, 10, 1)]})], iou=0.3)
    # inter 2, union 4 at iou 0.5: equality matches
    s["equality"] = Scene([f({0: [(0, 0, 2, 2)]}), f({0: [(0, 0, 2, 1)]})], iou=0.5)
    # track 2 takes detection 0 (IoU 0.82), which the optimum would have left to track 1
    s["greedy"] = Scene([f({0: [(0, 0, 10, 10), (4, 0, 14, 10)]}),
                         f({0: [(3, 0, 13, 10), (6, 0, 16, 10)]})], iou=0.3)
    # row 0: one track, two detections of equal IoU; row 1: two tracks, one detection
    s["tie"] = Scene([f({0: [(10, 10, 20, 20)], 1: [(12, 10, 22, 20), (8, 10, 18, 20)]}),
                      f({0: [(12, 10, 22, 20), (8, 10, 18, 20)], 1: [(10, 10, 20, 20)]})], iou=0.3)
    cls_frames = [f({0: [(0, 0, 8, 8, 0.9, 3)]}), f({0: [(0, 0, 8, 8, 0.9, 5)]})]
    s["class_aware"] = Scene(cls_frames)
    s["class_blind"] = Scene(cls_frames, class_aware=False)
    s["nan_coordinate"] = Scene([f({0: [(0, 0, NAN, 8), (20, 0, 28, 8)], 1: [(0, NAN, 8, 8)]})])
    # row 0: 6 rows, k = 4; row 1: a negative count over real rows
    s["count"] = Scene([f({0: _grid(6), 1: _grid(3)}, {1: -2})])
    # the second frame's weak detections: the first matches, the second is not born; nor is a NaN score
    s["min_score"] = Scene([f({0: [(0, 0, 8, 8, 0.9)]}),
                            f({0: [(1, 0, 9, 8, 0.1), (20, 0, 28, 8, 0.1), (40, 0, 48, 8, NAN)]})], min_score=0.5)
    s["nan_score"] = Scene([f({0: [(0, 0, 8, 8, NAN), (20, 0, 28, 8, 0.0)]})])
    # born, missed twice (dies on the second), then the slot is taken again under a fresh id
    s["max_age"] = Scene([f({0: [(0, 0, 8, 8)]}), f({}), f({}), f({0: [(0, 0, 8, 8)]})], max_age=1)
    # 4 tracks in 5 slots, then 4 boxes elsewhere: one is born, three are refused
    s["full_table"] = Scene([f({0: _grid(4)}), f({0: _grid(4, x0=100)})])
    s["label_mod"] = Scene([f({0: _grid(4)})], label_mod=3)
    return s


SCRIPTED = _scripted()


def random_walk(seed, batch=B, frames=12, k=6, tracks=7, max_det=8, busy=None, **kw):
    """Boxes that drift, appear and vanish, on a half-pixel grid (equal IoUs do occur), two classes,
    in shuffled order; row b is busier than row b-1 (``busy``: the chance of one more box, for
    every row and frame), counts go past ``k`` and now and then a coordinate is NaN."""
    rng = random.Random(seed)
    objs = [[] for _ in range(batch)]
    out = []
    for fi in range(frames):
        rows_by_b = {}
        for b in range(batch):
            objs[b] = [o for o in objs[b] if rng.random() > 0.15]
            p = 0.9 if fi == 0 else (0.3 + 0.6 * b / max(batch - 1, 1))
            p = p if busy is None else busy
            while len(objs[b]) < max_det and rng.random() < p:
                objs[b].append([rng.randrange(0, 400) / 2, rng.randrange(0, 240) / 2, rng.randrange(32, 120) / 2,
                                rng.randrange(32, 120) / 2, rng.randrange(-6, 7) / 2, rng.randrange(-6, 7) / 2,
                                rng.randrange(2)])
            rows = []
            for o in objs[b]:
                o[0] += o[4]
                o[1] += o[5]
                x1 = o[0] + rng.choice((-0.5, 0.0, 0.5))
                x2 = NAN if rng.random() < 0.04 else o[0] + o[2]
                rows.append((x1, o[1], x2, o[1] + o[3], rng.randrange(200, 960) / 1000, o[6]))
            rng.shuffle(rows)
            rows_by_b[b] = rows
        out.append(frame(rows_by_b, batch=batch, max_det=max_det))
    return Scene(out, k=k, tracks=tracks, **kw)


WALK_SEED = 0
WALK = random_walk(WALK_SEED, max_age=2, min_score=0.25)
# every lane a live track, every lane a detection; and the smallest table there is
WALK_FULL = random_walk(1, batch=2, frames=4, k=64, tracks=64, max_det=64, busy=0.995, max_age=1)
WALK_ONE = random_walk(17, batch=2, frames=6, k=1, tracks=1, max_det=1, max_age=1)


@functools.lru_cache(maxsize=None)
def _reference(scene_id):
    from aiko_services_amd.ops.reference import track_ref
    from aiko_services_amd.ops.track import new_state
    scene = _SCENES[scene_id]
    state = new_state(scene.batch, scene.tracks, "cpu")
    steps = []
    for det, count in scene.frames:
        ids, hits, labels, state = track_ref(det, count, state, scene.k, **scene.kw)
        steps.append((ids, hits, labels, state))
    return tuple(steps)


_SCENES = {}


def reference(scene):
    """``((ids, hits, labels, state_out), ...)`` of ``track_ref``, one per frame of ``scene``;
    computed once, not to be modified."""
    _SCENES[id(scene)] = scene
    return _reference(id(scene))
