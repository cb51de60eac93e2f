"""The tracker's rules, pinned on the CPU reference (``ops.reference.track_ref``): one scripted scene
per rule (track_scenes.py) with the values worked out by hand, and the seeded random walk that
test_gpu_track.py steps on the device.  No GPU needed."""
import numpy as np
import pytest
import torch

import track_scenes as S
from track_scenes import B, K, T


def _steps(name):
    return S.reference(S.SCRIPTED[name])


def _row(step, b, k=K):
    ids, hits, labels, _ = step
    return ids.view(-1, k)[b].tolist(), hits.view(-1, k)[b].tolist(), labels.view(-1, k)[b].tolist()


def test_shapes_and_empty_state():
    from aiko_services_amd.ops.track import TrackState, new_state
    state = new_state(B, T, "cpu")
    assert isinstance(state, TrackState)
    assert state.boxes.shape == (B, T, 4) and state.boxes.dtype == torch.float32
    assert state.meta.shape == (B, T, 4) and state.meta.dtype == torch.int32
    assert state.issued.shape == (B,) and state.issued.dtype == torch.int32
    assert not state.boxes.any() and not state.meta.any() and not state.issued.any()
    ids, hits, labels, out = _steps("equality")[0]
    for t in (ids, hits, labels):
        assert t.shape == (B * K,) and t.dtype == torch.int32
    assert out.boxes.shape == (B, T, 4) and out.meta.dtype == torch.int32 and out.issued.dtype == torch.int32


def test_reference_leaves_its_inputs_alone():
    from aiko_services_amd.ops.reference import track_ref
    scene = S.SCRIPTED["greedy"]
    state = S.reference(scene)[0][3]
    det, count = scene.frames[1]
    before = [t.clone() for t in (det, count, *state)]
    track_ref(det, count, state, scene.k, **scene.kw)
    assert all(torch.equal(a, b) for a, b in zip(before, (det, count, *state)))


def test_threshold_is_tested_in_fp64():
    # inter 3, union 10: the fp32 product rounds to 3.0 and would match; the fp64 product is above
    thr = np.float32(0.3)
    assert not 3.0 >= float(thr) * 10.0
    assert np.float32(3.0) >= thr * np.float32(10.0)
    first, second = _steps("threshold_fp64")
    assert _row(first, 0)[0] == [1, 0, 0, 0]
    assert _row(second, 0) == ([2, 0, 0, 0], [1, 0, 0, 0], [2, -1, -1, -1])
    assert second[3].meta[0, 0].tolist() == [1, 0, 1, 1] and second[3].meta[0, 1].tolist() == [2, 0, 1, 0]
    assert second[3].issued.tolist() == [2, 0, 0]


def test_equality_matches():
    second = _steps("equality")[1]
    assert _row(second, 0) == ([1, 0, 0, 0], [2, 0, 0, 0], [1, -1, -1, -1])
    assert second[3].boxes[0, 0].tolist() == [0, 0, 2, 1] and second[3].meta[0, 0].tolist() == [1, 0, 2, 0]


def test_greedy_not_optimal():
    first, second = _steps("greedy")
    assert _row(first, 0)[0] == [1, 2, 0, 0]
    assert _row(second, 0)[0] == [2, 3, 0, 0] and _row(second, 0)[1] == [2, 1, 0, 0]
    meta = second[3].meta[0]
    assert meta[0].tolist() == [1, 0, 1, 1]                # track 1: left out, one miss
    assert meta[1].tolist() == [2, 0, 2, 0] and meta[2].tolist() == [3, 0, 1, 0]
    assert second[3].boxes[0, 0].tolist() == [0, 0, 10, 10] and second[3].boxes[0, 1].tolist() == [3, 0, 13, 10]


def test_ties_go_to_the_lower_slot_then_the_lower_detection():
    second = _steps("tie")[1]
    assert _row(second, 0)[0] == [1, 2, 0, 0]              # one track, two detections: the lower index
    assert _row(second, 1)[0] == [1, 0, 0, 0]              # two tracks, one detection: the lower slot
    assert second[3].meta[1, 0].tolist() == [1, 0, 2, 0] and second[3].meta[1, 1].tolist() == [2, 0, 1, 1]


def test_class_decides_unless_class_blind():
    aware, blind = _steps("class_aware")[1], _steps("class_blind")[1]
    assert _row(aware, 0)[0] == [2, 0, 0, 0]
    assert aware[3].meta[0, :2].tolist() == [[1, 3, 1, 1], [2, 5, 1, 0]]
    assert _row(blind, 0)[0] == [1, 0, 0, 0]
    assert blind[3].meta[0, :2].tolist() == [[1, 5, 2, 0], [0, 0, 0, 0]]


def test_nan_coordinate_below_count_is_invalid():
    (step,) = _steps("nan_coordinate")
    assert _row(step, 0) == ([0, 1, 0, 0], [0, 1, 0, 0], [-1, 1, -1, -1])
    assert _row(step, 1)[0] == [0, 0, 0, 0] and not step[3].meta[1].any() and step[3].issued.tolist() == [1, 0, 0]
    assert step[3].boxes[0, 0].tolist() == [20, 0, 28, 8]


def test_count_is_truncated_to_k_and_negative_is_zero():
    (step,) = _steps("count")
    assert _row(step, 0)[0] == [1, 2, 3, 4] and step[3].issued.tolist() == [4, 0, 0]
    assert not step[3].meta[0, 4].any()                    # rows 4 and 5 were not born
    assert _row(step, 1) == ([0] * K, [0] * K, [-1] * K) and not step[3].meta[1].any()


def test_min_score_blocks_a_birth_but_not_a_match():
    second = _steps("min_score")[1]
    assert _row(second, 0) == ([1, 0, 0, 0], [2, 0, 0, 0], [1, -1, -1, -1])
    assert second[3].issued.tolist() == [1, 0, 0] and second[3].boxes[0, 0].tolist() == [1, 0, 9, 8]
    (step,) = _steps("nan_score")                          # min_score 0: score 0 is born, NaN is not
    assert _row(step, 0)[0] == [0, 1, 0, 0]


def test_max_age_death_and_slot_reuse_under_a_fresh_id():
    born, miss1, miss2, again = _steps("max_age")
    assert born[3].meta[0, 0].tolist() == [1, 0, 1, 0]
    assert miss1[3].meta[0, 0].tolist() == [1, 0, 1, 1] and miss1[3].boxes[0, 0].tolist() == [0, 0, 8, 8]
    assert not miss2[3].meta[0].any() and not miss2[3].boxes[0].any()      # a free slot is all zeros
    assert miss2[3].issued.tolist() == [1, 0, 0]
    assert _row(again, 0)[0] == [2, 0, 0, 0] and again[3].meta[0, 0].tolist() == [2, 0, 1, 0]


def test_full_table_refuses_births():
    first, second = _steps("full_table")
    assert _row(first, 0)[0] == [1, 2, 3, 4]
    assert _row(second, 0) == ([5, 0, 0, 0], [1, 0, 0, 0], [5, -1, -1, -1])
    assert second[3].meta[0, :, 0].tolist() == [1, 2, 3, 4, 5] and second[3].meta[0, :4, 3].tolist() == [1] * 4
    assert second[3].issued.tolist() == [5, 0, 0]


def test_labels_are_ids_modulo_label_mod():
    (step,) = _steps("label_mod")
    assert _row(step, 0)[0] == [1, 2, 3, 4] and _row(step, 0)[2] == [1, 2, 0, 1]


@pytest.mark.parametrize("name", sorted(S.SCRIPTED))
def test_a_row_without_detections_keeps_the_empty_state(name):
    for ids, hits, labels, state in _steps(name):
        assert _row((ids, hits, labels, state), 2) == ([0] * K, [0] * K, [-1] * K)
        assert not state.boxes[2].any() and not state.meta[2].any() and int(state.issued[2]) == 0


def walk_events(scene, steps):
    """What the scene exercises, from the reference's states alone."""
    ev = dict(births=0, long_matches=0, deaths=0, refused=0, reuses=0)
    had_id = torch.zeros(scene.batch, scene.tracks, dtype=torch.bool)
    prev = torch.zeros(scene.batch, scene.tracks, dtype=torch.int32)
    issued = torch.zeros(scene.batch, dtype=torch.int32)
    floor = scene.kw.get("min_score", 0.0)
    for (det, count), (ids, hits, _, state) in zip(scene.frames, steps):
        now = state.meta[:, :, 0]
        ev["births"] += int((state.issued - issued).sum())
        ev["long_matches"] += int((hits >= 3).sum())
        ev["deaths"] += int(((prev != 0) & (now == 0)).sum())
        ev["reuses"] += int(((now != 0) & (now != prev) & had_id).sum())
        i = torch.arange(scene.k)[None, :]
        valid = (i < count.clamp(0, scene.k)[:, None]) & torch.isfinite(det[:, :scene.k, :4]).all(-1)
        ev["refused"] += int((valid & (det[:, :scene.k, 4] >= floor) & (ids.view(-1, scene.k) == 0)).sum())
        had_id |= now != 0
        prev, issued = now, state.issued
    return ev


def test_random_walk_covers_the_rules():
    scene = S.WALK
    assert (scene.batch, len(scene.frames), scene.k, scene.tracks) == (3, 12, 6, 7)
    steps = S.reference(scene)
    ev = walk_events(scene, steps)
    print(f"random walk, seed {S.WALK_SEED}: {ev}")
    assert all(v >= 1 for v in ev.values()), ev
    # ids are unique per row and never come back
    seen = [set() for _ in range(scene.batch)]
    prev = torch.zeros(scene.batch, scene.tracks, dtype=torch.int32)
    for _, _, _, state in steps:
        now = state.meta[:, :, 0]
        for b in range(scene.batch):
            live = [i for i in now[b].tolist() if i]
            assert len(live) == len(set(live))
            fresh = set(live) - set(prev[b].tolist())
            assert not fresh & seen[b]
            seen[b] |= fresh
        free = now == 0
        assert not state.meta[free].any() and not state.boxes[free].any()
        prev = now
