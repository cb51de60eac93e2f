"""The scene of the redaction tests (``ops/redact.py``), shared by test_redact_reference.py (what
``redact_detections_ref`` must give, and what the scene must cover) and test_gpu_redact.py (the
kernel against ``redact_detections_ref``).  A configuration's reference is computed once per
process and handed out unchanged.

Three frames of 70 x 150 (150: the byte path; 148, a multiple of 4: the dword path), so that both
dimensions of the kernel's 128 x 32 tile are partial; ``max_det`` = 6, counts [0, 5, 2], the class
of row ``i`` is ``i``.

A plain module (no fixtures, no device requirement), like kernel_guard.py."""
from __future__ import annotations

import torch

B, H, W = 3, 70, 150
W4 = 148
MAX_DET, K = 6, 5
COUNTS = [0, 5, 2]
TILE_W, TILE_H = 128, 32       # pixels per workgroup of redact_detections_kernel (RD_TW, RD_TH)
CHUNK = 256                    # detection rows culled per round (RD_CHUNK)
BLOCKS = (4, 8, 16, 32)
NAN = float("nan")
FILL = (200, 17, 96)
SELECT_N = 5                   # length of the select table
SELECT_CLASSES = [0, 1, 3]     # ... which leaves row 4 of frame 1 (class 4) alone

# (x1, y1, x2, y2) per frame; rows past the list are the detector's padding (zeros, class -1)
BOXES = [
    [(10.0, 10.0, 60.0, 50.0)],                     # count 0: never used
    [(60.2, 30.5, 100.7, 52.1),                     # straddles the tile rows at y = 32
     (120.3, 3.6, 149.7, 30.9),                     # crosses x = 128, reaches the right edge's partial cells
     (NAN, NAN, 20.0, 20.0),                        # NaN row below count: not used
     (130.5, 50.25, 149.5, 69.75),                  # the bottom-right partial cells, both ways
     (3.3, 2.2, 30.9, 20.1)],
    [(70.0, 40.0, 110.0, 64.0),                     # these two overlap,
     (100.0, 50.0, 150.0, 70.0)],                   # and this one ends at the tensor's last byte
]


def det(boxes=BOXES):
    d = torch.zeros(B, MAX_DET, 6)
    d[:, :, 5] = -1
    for b, rows in enumerate(boxes):
        for i, r in enumerate(rows):
            d[b, i] = torch.tensor([*r, 0.9 - 0.1 * i, float(i)])
    return d


def frames(seed=0, width=W):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, width, 3), dtype=torch.uint8, generator=g)


def labels(k=K, seed=0):
    """A class per ROI slot, int32 ``[B*k]``.  Seed 0 (the shared scene): frame 1 = [4, 0, 9, -1, 1]
    (deselected, selected, the NaN row, negative, selected), frame 2 = [7, 3] (past the table,
    selected), so that under the select table the labels choose other rows than the detector's
    classes do; other seeds: random classes in [0, SELECT_N)."""
    g = torch.Generator().manual_seed(200 + seed)
    lab = torch.randint(0, SELECT_N, (B, MAX_DET), generator=g).to(torch.int32)
    if seed == 0:
        lab[1, :5] = torch.tensor([4, 0, 9, -1, 1], dtype=torch.int32)
        lab[2, :2] = torch.tensor([7, 3], dtype=torch.int32)
    return lab[:, :k].reshape(-1).contiguous()


def select_table():
    from aiko_services_amd.ops.redact import class_select
    return class_select(SELECT_CLASSES, SELECT_N)


_SCENE = {}


def scene():
    """Host inputs shared by the tests (made once, never modified)."""
    if not _SCENE:
        _SCENE.update(frames=frames(), frames4=frames(width=W4), det=det(),
                      count=torch.tensor(COUNTS, dtype=torch.int32), select=select_table(), labels=labels())
    return _SCENE


def inputs(width=W):
    s = scene()
    return s["frames" if width == W else "frames4"], s["det"], s["count"]


def selected_rects(width=W, k=K, margin=0.0, with_select=False, with_labels=False, det_=None, count=None,
                   labels_=None):
    """{frame: [(row, (X0, Y0, X1, Y1)), ...]}: the rects of the used and selected rows, from
    ``roi_rects_ref`` and the selection rule (not from ``redact_detections_ref``)."""
    from aiko_services_amd.ops.reference import roi_rects_ref
    s = scene()
    det_ = s["det"] if det_ is None else det_
    count = s["count"] if count is None else count
    lab = (labels(k) if labels_ is None else labels_) if with_labels else None
    table = s["select"] if with_select else None
    rects = roi_rects_ref(det_, count, k, (H, width), margin).view(det_.shape[0], k, 4).tolist()
    out = {}
    for b in range(det_.shape[0]):
        out[b] = []
        for i in range(k):
            x0, y0, x1, y1 = rects[b][i]
            if x1 <= x0:
                continue
            if table is not None:
                c = int(lab[b * k + i]) if lab is not None else int(det_[b, i, 5])
                if not (0 <= c < table.shape[0] and int(table[c])):
                    continue
            out[b].append((i, (x0, y0, x1, y1)))
    return out


def coverage(width=W, **kw):
    """bool ``[B, H, width]``: the pixels inside at least one rect of :func:`selected_rects`."""
    mask = torch.zeros(B, H, width, dtype=torch.bool)
    for b, rows in selected_rects(width, **kw).items():
        for _, (x0, y0, x1, y1) in rows:
            mask[b, y0:y1, x0:x1] = True
    return mask


_REF = {}


def reference(width=W, block=16, mode="pixelate", with_select=False, with_labels=False, margin=0.0, k=K):
    """``redact_detections_ref`` on the shared scene, computed once per configuration; not to be
    modified."""
    key = (width, block, mode, with_select, with_labels, margin, k)
    if key not in _REF:
        from aiko_services_amd.ops.reference import redact_detections_ref
        s = scene()
        _REF[key] = redact_detections_ref(*inputs(width), k, mode=mode, block=block, fill=FILL, margin=margin,
                                          select=s["select"] if with_select else None,
                                          labels=labels(k) if with_labels else None)
    return _REF[key]
