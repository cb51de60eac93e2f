"""Object identity across frames (``csrc/kernels/track_ops.hip``): a greedy IoU tracker over the
detector's fixed-size NMS rows.  Batch row ``b`` is one camera; its table of ``T`` track slots is a
:class:`TrackState` in HBM, read and rewritten by one launch per frame.  Rows, counts and the table
are read by the kernel: no host copy, no synchronisation, hipGraph-capturable like
:func:`~aiko_services_amd.ops.roi.roi_crop`.

The rules, per row and step (:func:`~aiko_services_amd.ops.reference.track_ref` is the same in
plain loops and equals the kernel bit for bit):

1. Detection ``i`` is valid iff ``i < min(max(count[b], 0), k)`` and its four coordinates are
   finite (the rule of ``roi_crop`` and ``draw_detections``); its class is ``det[b, i, 5]`` as an
   int (NaN -> 0, clamped to int32).  Rows at or past ``count[b]`` are never read.
2. Pair geometry in fp32, every operation rounded on its own: ``aw = ax2 - ax1``, ``ah = ay2 -
   ay1``, ``area_a = aw * ah`` (the same for b); ``iw = max(min(ax2, bx2) - max(ax1, bx1), 0)``,
   ``ih`` likewise, ``inter = iw * ih``; ``union = (area_a + area_b) - inter``.
3. A pair (live track, valid detection) is eligible iff the classes are equal (``class_aware``),
   ``inter > 0``, ``union > 0`` and ``inter >= iou * union`` — that product in fp64 of the fp32
   values, which is exact.
4. Greedy matching: the eligible pairs in order of IoU, highest first (``inter_p * union_q >
   inter_q * union_p`` in fp64, exact), ties to the lower track slot, then to the lower detection
   index; a pair matches iff its track and its detection are both still unmatched.
5. A matched track takes the detection's box, ``hits += 1``, ``missed = 0`` (and the detection's
   class without ``class_aware``).
6. An unmatched live track: ``missed += 1``; past ``max_age`` its slot becomes free.
7. Then, in index order, every unmatched valid detection with ``score >= min_score`` (fp32; a NaN
   score never) takes the lowest free slot: ``issued[b] += 1``, ``id = issued[b]``, ``hits = 1``.
   With no free slot it stays untracked.
8. Per ROI slot ``b*k + i``: ``ids`` (0 if invalid or untracked), ``hits`` and ``labels`` = ``id %
   label_mod`` (-1 without a track: ``draw_detections`` draws it in ``palette[0]``, no name).

A slot is free iff its id is 0, and a free slot is all zeros: the empty state is all zeros.  Ids
are unique per row and never reused.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

__all__ = ["TrackState", "new_state", "track_detections"]


class TrackState(NamedTuple):
    """``boxes`` fp32 ``[B, T, 4]``, ``meta`` int32 ``[B, T, 4]`` = (id, cls, hits, missed),
    ``issued`` int32 ``[B]``: ids handed out so far."""
    boxes: torch.Tensor
    meta: torch.Tensor
    issued: torch.Tensor


def new_state(B: int, T: int, device="cuda") -> TrackState:
    """The empty state of ``B`` rows x ``T`` track slots: zeros."""
    return TrackState(torch.zeros(B, T, 4, dtype=torch.float32, device=device),
                      torch.zeros(B, T, 4, dtype=torch.int32, device=device),
                      torch.zeros(B, dtype=torch.int32, device=device))


def track_detections(det: torch.Tensor, count: torch.Tensor, state: TrackState, k: int, *, iou: float = 0.3,
                     max_age: int = 30, min_score: float = 0.0, class_aware: bool = True, label_mod: int = 1000,
                     state_out: TrackState | None = None, ids: torch.Tensor | None = None,
                     hits: torch.Tensor | None = None, labels: torch.Tensor | None = None):
    """One tracker step: ``det`` ``[B, max_det, 6]`` / ``count`` ``[B]`` (the outputs of
    :func:`~aiko_services_amd.ops.detect.topk_nms`) and ``state`` -> ``(ids, hits, labels,
    state_out)``, the first three int32 ``[B*k]`` (slot ``b*k + i`` belongs to row ``i`` of frame
    ``b``, the layout of ``draw_detections(labels=...)``).  ``1 <= k <= min(max_det, 64)``, ``1 <=
    T <= 64``.  ``state`` is only read; ``state_out`` (new by default) must be another allocation.
    Every element of every output is written."""
    B, T = state.boxes.shape[0], state.boxes.shape[1]
    dev = det.device
    if state_out is None:
        state_out = TrackState(torch.empty(B, T, 4, dtype=torch.float32, device=dev),
                               torch.empty(B, T, 4, dtype=torch.int32, device=dev),
                               torch.empty(B, dtype=torch.int32, device=dev))
    ids, hits, labels = (torch.empty(B * int(k), dtype=torch.int32, device=dev) if t is None else t
                         for t in (ids, hits, labels))
    torch.ops.aiko.track_detections_out(det, count, state.boxes, state.meta, state.issued, int(k), float(iou),
                                        int(max_age), float(min_score), bool(class_aware), int(label_mod),
                                        state_out.boxes, state_out.meta, state_out.issued, ids, hits, labels)
    return ids, hits, labels, state_out
