"""Detection overlay on the MI355X (``overlay_ops.hip``): bit for bit against the painter's
reference (``draw_detections_ref``), in place, the device-side count under hipGraph replay, guard
bands, refusals, and the DetectionOverlay element in the example pipelines against the same
kernels called directly."""
import json
import queue
from pathlib import Path

import numpy as np
import pytest
import torch

from kernel_guard import guarded

pytestmark = pytest.mark.gpu

B, H, W = 3, 70, 150
W4 = 148                       # a multiple of 4: the dword store path (150: the byte path)
MAX_DET = 6
TILE_W, TILE_H = 128, 32       # pixels per workgroup of draw_detections_kernel (OV_TW, OV_TH)
CHUNK = 256                    # detection rows culled per round (OV_CHUNK)
GW = 5
NAN = float("nan")
COUNTS = [0, 6, 2]             # nothing drawn / truncated to K, with a NaN row / partial
NAMES = ["cat", "person", "a", "", "zz9_x"]
NAME_W = 6
CASES = [(4, 1, 1), (6, 2, 3), (6, 1, 16)]      # (K, text_scale, thickness)

# (x1, y1, x2, y2) per frame; rows past the list are the detector's padding (zeros, class -1)
BOXES = [
    [(10.0, 10.0, 60.0, 50.0)],                     # count 0: never used
    [(0.0, 0.0, 150.0, 70.0),                       # the whole frame: under every other row's pixels
     (60.2, 30.5, 100.7, 52.1),
     (120.3, 3.6, 149.7, 30.9),                     # no room above; a wide label is pushed left
     (NAN, NAN, 20.0, 20.0),                        # NaN row below count: not drawn
     (130.5, 50.25, 149.5, 69.75),                  # bottom-right corner, narrower than its label
     (3.3, 2.2, 30.9, 20.1)],
    [(70.0, 40.0, 110.0, 64.0),
     (100.0, 50.0, 150.0, 70.0)],                   # its outline ends at the tensor's last byte
]


def _det(boxes=BOXES):
    det = torch.zeros(B, MAX_DET, 6)
    det[:, :, 5] = -1
    for b, rows in enumerate(boxes):
        for i, r in enumerate(rows):
            det[b, i] = torch.tensor([*r, 0.9 - 0.1 * i, float(i)])
    return det


def _frames(seed=0, width=W):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, width, 3), dtype=torch.uint8, generator=g)


def _slots(k, seed=0):
    """labels / scores per ROI slot: -1, a class past the name table (5, 99), classes that wrap the
    7-entry palette (7..12), probabilities outside [0, 1] and a NaN among the used slots."""
    g = torch.Generator().manual_seed(100 + seed)
    labels = torch.randint(0, 13, (B, MAX_DET), generator=g).to(torch.int32)
    scores = torch.rand(B, MAX_DET, generator=g)
    labels[1, :6] = torch.tensor([8, -1, 12, 3, 2, 7], dtype=torch.int32)
    labels[2, :2] = torch.tensor([99, 5], dtype=torch.int32)
    scores[1, 0], scores[1, 1], scores[1, 2], scores[2, 0] = 0.005, 1.7, NAN, -0.2
    return labels[:, :k].reshape(-1).contiguous(), scores[:, :k].reshape(-1).contiguous()


_SCENE = {}


def scene():
    """Host inputs shared by the tests (made once, never modified)."""
    if not _SCENE:
        from aiko_services_amd.ops.overlay import pack_names
        rng = np.random.default_rng(0)
        font = torch.from_numpy((rng.integers(0, 256, (95, 7)) & 0xF8).astype(np.uint8))
        palette = torch.from_numpy(rng.integers(0, 256, (7, 3)).astype(np.uint8))
        _SCENE.update(frames=_frames(), frames4=_frames(width=W4), det=_det(),
                      count=torch.tensor(COUNTS, dtype=torch.int32), names=pack_names(NAMES, NAME_W),
                      font=font, palette=palette)
    return _SCENE


def _inputs(width=W):
    s = scene()
    return s["frames" if width == W else "frames4"], s["det"], s["count"]


def _tables():
    s = scene()
    return s["names"], s["font"], s["palette"]


_REF = {}


def reference(width, k, s, t, with_slots, show):
    """The painter's reference for the shared scene, computed once per configuration."""
    key = (width, k, s, t, with_slots, show)
    if key not in _REF:
        from aiko_services_amd.ops.reference import draw_detections_ref
        labels, scores = _slots(k) if with_slots else (None, None)
        _REF[key] = draw_detections_ref(*_inputs(width), k, *_tables(), labels=labels, scores=scores, thickness=t,
                                        text_scale=s, show_score=show, glyph_width=GW)
    return _REF[key]


def run(frames, det, count, k, s, t, labels=None, scores=None, show=True, tables=None, out=None, margin=0.0):
    from aiko_services_amd.ops.overlay import draw_detections
    dev = lambda x: None if x is None else x.cuda()  # noqa: E731
    names, font, palette = tables or _tables()
    res = draw_detections(frames.cuda(), dev(det), dev(count), k, dev(names), dev(font), dev(palette),
                          labels=dev(labels), scores=dev(scores), thickness=t, text_scale=s, margin=margin,
                          show_score=show, glyph_width=GW, out=out)
    torch.cuda.synchronize()
    return res.cpu()


# ---- the geometry of the scene, from the definition (not from the kernel) -------------------

def _geometry(width, k, s, t, with_slots, show):
    """Per used row: (frame, index, rect, label rect or None, shifted_left, above)."""
    from aiko_services_amd.ops.reference import overlay_text_ref, roi_rects_ref
    _, det, count = _inputs(width)
    names = _tables()[0]
    labels, scores = _slots(k) if with_slots else (None, None)
    rects = roi_rects_ref(det, count, k, (H, width), 0.0).view(B, k, 4).tolist()
    rows = []
    for b in range(B):
        for i in range(k):
            x0, y0, x1, y1 = rects[b][i]
            if x1 <= x0:
                continue
            c = int(labels[b * k + i]) if with_slots else int(det[b, i, 5])
            p = scores[b * k + i] if with_slots else det[b, i, 4]
            n = len(overlay_text_ref(c, p, names, show))
            lab, shifted, above = None, False, False
            if n:
                lw, lh = n * GW * s + 2 * s, 7 * s + 2 * s
                lx = max(min(x0, width - lw), 0)
                ly = y0 - lh if y0 - lh >= 0 else y0
                lab = (lx, ly, min(lx + lw, width), min(ly + lh, H))
                shifted, above = lx < x0, ly < y0
            rows.append((b, i, (x0, y0, x1, y1), lab, shifted, above))
    return rows


def _touches(r, tile):
    return r is not None and r[0] < tile[2] and r[2] > tile[0] and r[1] < tile[3] and r[3] > tile[1]


def _tile_lists(width, k, s, t, with_slots, show):
    """{(frame, tile y, tile x): [row index, ...]}: the rows a tile must look at — those whose label
    or outline has a pixel in it."""
    rows = _geometry(width, k, s, t, with_slots, show)
    lists = {}
    for b in range(B):
        for ty in range(0, H, TILE_H):
            for tx in range(0, width, TILE_W):
                tile = (tx, ty, min(tx + TILE_W, width), min(ty + TILE_H, H))
                keep = []
                for fb, i, r, lab, _, _ in rows:
                    if fb != b:
                        continue
                    inside = tile[0] >= r[0] + t and tile[2] <= r[2] - t and tile[1] >= r[1] + t and \
                        tile[3] <= r[3] - t
                    if _touches(lab, tile) or (_touches(r, tile) and not inside):
                        keep.append(i)
                lists[(b, ty // TILE_H, tx // TILE_W)] = keep
    return lists


def test_scene_covers_the_tile_paths():
    assert W > TILE_W and W % TILE_W and H > TILE_H and H % TILE_H      # > 1 tile each way, partial last tiles
    assert W4 > TILE_W and W4 % TILE_W and W4 % 4 == 0 and W % 4
    assert MAX_DET < CHUNK                                              # one culling round
    for k, s, t in CASES:
        lists = _tile_lists(W, k, s, t, False, True)
        used = {b: {i for fb, i, *_ in _geometry(W, k, s, t, False, True) if fb == b} for b in range(B)}
        assert not used[0] and len(used[1]) == k - 1 and len(used[2]) == 2           # the NaN row is not drawn
        # a tile with nothing to draw (at the small labels also in a frame that has boxes), and a tile
        # that sees every used row of its frame
        assert any(not rows for rows in lists.values()), (k, s, t)
        assert s > 1 or any(not rows for (b, _, _), rows in lists.items() if used[b]), (k, s, t)
        assert any(len(rows) >= 2 and set(rows) == used[b] for (b, _, _), rows in lists.items()), (k, s, t)
    geo = _geometry(W, 4, 1, 1, False, True)
    placed = [above for _, _, _, lab, _, above in geo if lab is not None]
    assert any(placed) and not all(placed)                             # labels above and inside their boxes
    shifted = [(b, i) for b, i, _, lab, sh, _ in _geometry(W, 6, 2, 3, False, True) if sh]
    assert shifted == [(1, 1), (1, 2), (1, 4), (2, 1)]                 # labels pushed left by the frame's edge
    # row 0 of frame 1 covers the whole frame: every other row of that frame lies on top of nothing
    # but row 0's interior, and its outline beats theirs wherever they meet it
    assert geo[0][:3] == (1, 0, (0, 0, W, H))
    # thickness 16 exceeds half of a small box: the outline is the whole rect
    small = [r for b, i, r, *_ in _geometry(W, 6, 1, 16, False, True) if r[2] - r[0] <= 32 or r[3] - r[1] <= 32]
    assert small


def _check_reference_shows(width, k, s, t, with_slots, show):
    """The reference's picture has what the geometry promises: each row's outline corner or label
    corner carries the row's colour unless a lower row covers that pixel."""
    ref = reference(width, k, s, t, with_slots, show)
    frames, det, _ = _inputs(width)
    palette = _tables()[2]
    labels, _ = _slots(k) if with_slots else (None, None)
    rows = _geometry(width, k, s, t, with_slots, show)
    assert (ref != frames).any()
    assert torch.equal(ref[0], frames[0])                                           # count 0
    for b, i, r, lab, _, _ in rows:
        c = int(labels[b * k + i]) if with_slots else int(det[b, i, 5])
        col = palette[c % 7 if c >= 0 else 0]
        for x, y in [(r[0], r[1])] + ([(lab[0], lab[1])] if lab else []):
            covered = any(fb == b and j < i and (_touches(l2, (x, y, x + 1, y + 1)) or
                                                (_touches(r2, (x, y, x + 1, y + 1)) and
                                                 (x < r2[0] + t or x >= r2[2] - t or y < r2[1] + t or y >= r2[3] - t)))
                          for fb, j, r2, l2, _, _ in rows)
            own_label = lab is not None and _touches(lab, (x, y, x + 1, y + 1))
            if not covered and (own_label or (x, y) == (r[0], r[1])):
                assert torch.equal(ref[b, y, x], col), (b, i, x, y)


@pytest.mark.parametrize("width", [W, W4])
@pytest.mark.parametrize("k,s,t", CASES)
def test_equals_reference(native, width, k, s, t):
    frames, det, count = _inputs(width)
    for with_slots in (False, True):
        labels, scores = _slots(k) if with_slots else (None, None)
        for show in (True, False):
            _check_reference_shows(width, k, s, t, with_slots, show)
            before = frames.clone()
            got = run(frames, det, count, k, s, t, labels, scores, show)
            ref = reference(width, k, s, t, with_slots, show)
            diff = (got != ref).any(-1)
            where = torch.nonzero(diff)[:5].tolist()
            print(f"overlay W={width} K={k} s={s} t={t} slots={with_slots} score={show}: "
                  f"{int(diff.sum())} of {diff.numel()} pixels differ {where}")
            assert torch.equal(got, ref)
            assert torch.equal(frames, before)


def test_margin_draws_the_rects_of_roi_crop(native):
    from aiko_services_amd.ops.reference import draw_detections_ref
    from aiko_services_amd.ops.roi import roi_crop
    frames, det, count = _inputs()
    got = run(frames, det, count, 6, 1, 2, margin=0.15)
    ref = draw_detections_ref(frames, det, count, 6, *_tables(), thickness=2, text_scale=1, margin=0.15,
                              glyph_width=GW)
    assert torch.equal(got, ref)
    _, rois = roi_crop(frames.cuda(), det.cuda(), count.cuda(), 6, (8, 8), 0.15)
    x0, y0, x1, y1 = rois.cpu()[1 * 6 + 1].tolist()                    # frame 1, row 1: under no other outline
    assert (x0, y0, x1, y1) == (54, 27, 107, 56)
    col = _tables()[2][1]
    assert (got[1, y0 + 20, x0:x0 + 2] == col).all() and (got[1, y0 + 20, x1 - 2:x1] == col).all()
    assert torch.equal(got[1, y0 + 20, x0 - 1], frames[1, y0 + 20, x0 - 1])
    assert torch.equal(got[1, y0 + 20, x1], frames[1, y0 + 20, x1])


@pytest.mark.parametrize("width", [W, W4])
def test_in_place_equals_out_of_place(native, width):
    from aiko_services_amd.ops.overlay import draw_detections
    frames, det, count = _inputs(width)
    names, font, palette = (x.cuda() for x in _tables())
    for k, s, t in CASES:
        labels, scores = (x.cuda() for x in _slots(k))
        buf = frames.cuda().clone()
        res = draw_detections(buf, det.cuda(), count.cuda(), k, names, font, palette, labels=labels, scores=scores,
                              thickness=t, text_scale=s, glyph_width=GW, out=buf)
        torch.cuda.synchronize()
        assert res is buf
        assert torch.equal(buf.cpu(), reference(width, k, s, t, True, True)), (k, s, t)


def test_unused_rows_and_slots_are_never_read(native):
    frames, det, count = _inputs()
    k, s, t = 4, 1, 1
    labels, scores = _slots(k)
    base = run(frames, det, count, k, s, t, labels, scores)
    assert torch.equal(base, reference(W, k, s, t, True, True))
    g = torch.Generator().manual_seed(3)
    for fill in ("nan", "garbage"):
        d, lab, sc = det.clone(), labels.clone().view(B, k), scores.clone().view(B, k)
        for b, c in enumerate(COUNTS):
            n = MAX_DET - c
            d[b, c:] = NAN if fill == "nan" else (torch.rand(n, 6, generator=g) - 0.5) * 1e4
            u = min(c, k)
            lab[b, u:] = -2 ** 31 if fill == "nan" else torch.randint(-10 ** 9, 10 ** 9, (k - u,), generator=g).int()
            sc[b, u:] = NAN if fill == "nan" else (torch.rand(k - u, generator=g) - 0.5) * 1e30
        d[1, 3] = det[1, 3]                                  # the NaN row below the count stays as it is
        d[1, 3, 4:] = NAN if fill == "nan" else 1e9         # ... but its score and class are never used
        lab[1, 3], sc[1, 3] = 10 ** 9, NAN
        got = run(frames, d, count, k, s, t, lab.reshape(-1), sc.reshape(-1))
        assert torch.equal(got, base), fill
    # rows at and past K are unused too, whatever the count says
    d = det.clone()
    d[:, k:] = NAN
    assert torch.equal(run(frames, d, count, k, s, t, labels, scores), base)


def test_device_side_count_under_graph_replay(native):
    from aiko_services_amd.ops.overlay import draw_detections
    from aiko_services_amd.ops.reference import roi_rects_ref
    K, s, t = 4, 1, 2
    frames, det, count = (x.cuda() for x in _inputs())
    names, font, palette = (x.cuda() for x in _tables())
    labels, scores = (x.cuda() for x in _slots(K))
    out = torch.empty_like(frames)
    kw = dict(thickness=t, text_scale=s, glyph_width=GW)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        draw_detections(frames, det, count, K, names, font, palette, labels=labels, scores=scores, out=out, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        draw_detections(frames, det, count, K, names, font, palette, labels=labels, scores=scores, out=out, **kw)
    first = None
    # the captured scene again, then two rewrites: frame 0 gets boxes, frame 1 loses them, frame 2
    # changes its boxes; then the reverse
    for step, (seed, counts, order) in enumerate([(0, COUNTS, [0, 1, 2]), (5, [2, 0, 5], [1, 2, 0]),
                                                  (6, [1, 3, 0], [2, 0, 1])]):
        frames.copy_(_frames(seed).cuda())
        det.copy_(_det([BOXES[i] for i in order]).cuda())
        count.copy_(torch.tensor(counts, dtype=torch.int32).cuda())
        labels.copy_(_slots(K, seed)[0].cuda())
        out.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        eager = draw_detections(frames.clone(), det.clone(), count.clone(), K, names, font, palette,
                                labels=labels.clone(), scores=scores, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, eager), step
        assert (out != frames).any()
        rois = roi_rects_ref(det.cpu(), count.cpu(), K, (H, W), 0.0)
        valid = rois[:, 2] > rois[:, 0]
        if first is None:
            first = valid
        else:
            assert (valid & ~first).any() and (~valid & first).any()     # slots flipped both ways


@pytest.mark.parametrize("width", [W, W4])
def test_guard_bands(native, width):
    from aiko_services_amd.ops.overlay import draw_detections
    K, s, t = 6, 2, 3
    frames, det, count = _inputs(width)
    names, font, palette = _tables()
    labels, scores = _slots(K)
    fresh = run(frames, det, count, K, s, t, labels, scores)
    assert torch.equal(fresh, reference(width, K, s, t, True, True))
    ops = {"frames": (frames, torch.uint8), "det": (det, torch.float32), "count": (count, torch.int32),
           "names": (names, torch.uint8), "font": (font, torch.uint8), "palette": (palette, torch.uint8),
           "labels": (labels, torch.int32), "scores": (scores, torch.float32)}
    g, checks = {}, []
    for name, (value, dtype) in ops.items():
        g[name], check = guarded(value.shape, dtype, "cuda", values=value, name=name)
        checks.append(check)
    go, co = guarded(frames.shape, torch.uint8, "cuda", name="out")
    draw_detections(g["frames"], g["det"], g["count"], K, g["names"], g["font"], g["palette"], labels=g["labels"],
                    scores=g["scores"], thickness=t, text_scale=s, glyph_width=GW, out=go)
    torch.cuda.synchronize()
    for check in checks + [co]:
        check()
    for name, (value, _) in ops.items():                                 # no input changed (bytes: NaNs inside)
        assert torch.equal(g[name].cpu().view(torch.uint8), value.contiguous().view(torch.uint8)), name
    assert torch.equal(go.cpu(), fresh)
    # the corner box of the last frame (slot label 5, colour 5): its outline ends at the tensor's
    # last byte, right in front of the 0xA5 guard
    col = palette[5]
    assert (go[-1, H - t:, width - 50 + 20:].cpu() == col).all() and (go[-1, 60:, width - t:].cpu() == col).all()
    # the same, drawn in place between the guards
    draw_detections(g["frames"], g["det"], g["count"], K, g["names"], g["font"], g["palette"], labels=g["labels"],
                    scores=g["scores"], thickness=t, text_scale=s, glyph_width=GW, out=g["frames"])
    torch.cuda.synchronize()
    for check in checks:
        check()
    assert torch.equal(g["frames"].cpu(), fresh)


def test_refusals(native):
    from aiko_services_amd.ops.overlay import draw_detections
    frames, det, count = (x.cuda() for x in _inputs())
    names, font, palette = (x.cuda() for x in _tables())
    K = 4
    labels, scores = (x.cuda() for x in _slots(K))

    def call(frames=frames, det=det, count=count, k=K, names=names, font=font, palette=palette, **kw):
        kw.setdefault("glyph_width", GW)
        return draw_detections(frames, det, count, k, names, font, palette, **kw)

    wide = torch.zeros(B, H, 2 * W, 3, dtype=torch.uint8, device="cuda")
    assert not wide[:, :, ::2].is_contiguous()
    for match, kw in [
            ("frames uint8", dict(frames=frames.float())),
            ("frames uint8", dict(frames=frames[..., :2].contiguous())),
            ("contiguous", dict(frames=wide[:, :, ::2])),
            ("det fp32", dict(det=det.double())),
            ("det fp32", dict(det=det[:, :, :5].contiguous())),
            ("det fp32", dict(det=det[:2])),
            ("contiguous", dict(det=det.transpose(0, 1).contiguous().transpose(0, 1))),
            ("count int32", dict(count=count.long())),
            ("count int32", dict(count=count[:2])),
            ("k <= max_det", dict(k=MAX_DET + 1)),
            ("k <= max_det", dict(k=0)),
            ("labels int32", dict(labels=labels.long())),
            ("labels int32", dict(labels=labels[:-1])),
            ("labels int32", dict(labels=labels.view(B, K))),
            ("scores fp32", dict(scores=scores.double())),
            ("scores fp32", dict(scores=torch.zeros(B * K + 1, device="cuda"))),
            ("names uint8", dict(names=names.int())),
            ("names uint8", dict(names=torch.zeros(5, 33, dtype=torch.uint8, device="cuda"))),
            ("names uint8", dict(names=torch.zeros(5, 0, dtype=torch.uint8, device="cuda"))),
            ("font uint8", dict(font=font.int())),
            ("font uint8", dict(font=torch.zeros(95, 17, dtype=torch.uint8, device="cuda"))),
            ("font uint8", dict(font=torch.zeros(95, 0, dtype=torch.uint8, device="cuda"))),
            ("glyph_width", dict(glyph_width=0)),
            ("glyph_width", dict(glyph_width=9)),
            ("palette uint8", dict(palette=torch.zeros(0, 3, dtype=torch.uint8, device="cuda"))),
            ("palette uint8", dict(palette=torch.zeros(7, 4, dtype=torch.uint8, device="cuda"))),
            ("palette uint8", dict(palette=palette.float())),
            ("thickness", dict(thickness=0)),
            ("thickness", dict(thickness=17)),
            ("text_scale", dict(text_scale=0)),
            ("text_scale", dict(text_scale=5)),
            ("margin", dict(margin=-0.1)),
            ("margin", dict(margin=float("inf"))),
            ("margin", dict(margin=NAN)),
            ("out uint8", dict(out=torch.empty(B, H, W + 1, 3, dtype=torch.uint8, device="cuda"))),
            ("out uint8", dict(out=torch.empty(B, H, W, 3, dtype=torch.int8, device="cuda"))),
            ("contiguous", dict(out=wide[:, :, ::2])),
            ("GPU tensor", dict(frames=frames.cpu())),
            ("GPU tensor", dict(names=names.cpu())),
            ("GPU tensor", dict(labels=labels.cpu())),
            ("GPU tensor", dict(out=torch.empty(B, H, W, 3, dtype=torch.uint8)))]:
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    # partial overlap: out starts one frame into the storage of frames
    big = torch.zeros(B + 1, H, W, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="overlaps"):
        call(frames=big[:B], out=big[1:])
    call(frames=big[:2], det=det[:2], count=count[:2], out=big[2:])           # adjacent, disjoint: fine
    with pytest.raises(RuntimeError, match="grid limit"):
        call(frames=torch.zeros(65536, 1, 1, 3, dtype=torch.uint8, device="cuda"),
             det=torch.zeros(65536, 1, 6, device="cuda"),
             count=torch.zeros(65536, dtype=torch.int32, device="cuda"), k=1)
    torch.cuda.synchronize()


def test_more_rows_than_one_culling_round(native):
    """300 rows per frame (the YOLO bench's max_det) take two culling rounds; the pixels a first
    round's row hit stay that row's.  One frame, boxes from a seed, every row used."""
    from aiko_services_amd.ops.reference import draw_detections_ref
    n, h, w = 300, 96, 260
    assert n > CHUNK
    g = torch.Generator().manual_seed(11)
    frames = torch.randint(0, 256, (1, h, w, 3), dtype=torch.uint8, generator=g)
    bw, bh = 4 + torch.rand(n, generator=g) * 60, 4 + torch.rand(n, generator=g) * 40
    x1, y1 = torch.rand(n, generator=g) * (w - bw), torch.rand(n, generator=g) * (h - bh)
    det = torch.stack([x1, y1, x1 + bw, y1 + bh, torch.rand(n, generator=g),
                       torch.randint(0, 9, (n,), generator=g).float()], -1)[None].contiguous()
    count = torch.tensor([n], dtype=torch.int32)
    got = run(frames, det, count, n, 1, 1)
    ref = draw_detections_ref(frames, det, count, n, *_tables(), thickness=1, text_scale=1, glyph_width=GW)
    late = draw_detections_ref(frames, det, torch.tensor([CHUNK], dtype=torch.int32), n, *_tables(), thickness=1,
                               text_scale=1, glyph_width=GW)
    assert (ref != late).any()                               # rows of the second round are visible
    assert torch.equal(got, ref)


# ---- the example pipelines ------------------------------------------------------------------

# conf 0.2987 on 240 x 320 noise frames keeps 1-3 boxes per frame of the seeded YOLOv8-n, so with 4
# slots some are used and some are empty (the threshold's derivation: test_gpu_roi.py)
PIPE_CONF = 0.2987
PIPE_K = 4
EXAMPLES = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/yolo"


def _definition(name, lanes):
    d = json.loads((EXAMPLES / name).read_text())
    d["parameters"]["gpu_lanes"] = lanes
    by_name = {e["name"]: e for e in d["elements"]}
    by_name["SyntheticFrames"]["parameters"].update(batch=2, height=240, width=320)
    by_name["YoloDetector"]["parameters"].update(autotune=False, graph=True, conf=PIPE_CONF)
    by_name["DetectionOverlay"]["parameters"].update(rois=PIPE_K)
    if "RoiCrop" in by_name:
        by_name["RoiCrop"]["parameters"].update(rois=PIPE_K)
        by_name["ResNet50Classifier"]["parameters"].update(autotune=False, graph=True)
    return d


def _run_pipeline(name, lanes, frames=3):
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    p = PipelineImpl.create_pipeline("<overlay>", parse_pipeline_definition_dict(_definition(name, lanes)),
                                     None, None, "c", [], 0, None, 60, queue_response=q)
    p.response_swag = True                     # the whole swag comes back, device tensors included
    # the element's output replaces ``images`` in the swag: keep what it was given
    element = p.pipeline_graph.get_node("DetectionOverlay").element
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
        assert swag["images"].data_ptr() != seen[-1].data_ptr()
        outs.append({"source": seen[i], "images": swag["images"].clone(), "det": swag["detections"].clone(),
                     "count": swag["counts"].clone()})
    assert p.share["gpu_lanes"] == lanes and len(seen) == frames
    return outs


def _element_tables(classes):
    from aiko_services_amd.ops.overlay import default_font, default_palette, pack_names
    font, gw = default_font()
    return pack_names([f"class_{i}" for i in range(classes)], 16), font, default_palette(20), gw


def test_overlay_pipeline_matches_direct_calls(native):
    from aiko_services_amd.models.resnet50 import ResNet50
    from aiko_services_amd.models.yolov8 import YOLOv8
    from aiko_services_amd.ops.overlay import draw_detections
    from aiko_services_amd.ops.reference import draw_detections_ref
    from aiko_services_amd.ops.roi import roi_crop
    from aiko_services_amd.ops.vision import softmax_topk
    one = _run_pipeline("yolo_overlay_gpu.json", 1)
    yolo = YOLOv8(scale="n", seed=0, device="cuda", conf=PIPE_CONF)
    resnet = ResNet50(seed=0, device="cuda")
    names, font, palette, gw = _element_tables(1000)
    dn, df, dp = names.cuda(), font.cuda(), palette.cuda()
    drawn = unused = 0
    for o in one:
        det, count = yolo.detect(o["source"])
        crops, rois = roi_crop(o["source"], det, count, PIPE_K, (224, 224), 0.0)
        logits = resnet.logits(crops)
        assert logits.shape == (2 * PIPE_K, 1000)
        prob, index = softmax_topk(logits, 1)
        direct = draw_detections(o["source"], det, count, PIPE_K, dn, df, dp, labels=index.view(-1),
                                 scores=prob.view(-1), glyph_width=gw)
        torch.cuda.synchronize()
        assert torch.equal(o["det"], det) and torch.equal(o["count"], count)
        assert torch.equal(o["images"], direct)
        ref = draw_detections_ref(o["source"], det, count, PIPE_K, names, font, palette, labels=index.view(-1).cpu(),
                                  scores=prob.view(-1).cpu(), glyph_width=gw)
        assert torch.equal(o["images"].cpu(), ref)
        valid = (rois[:, 2] > rois[:, 0]).cpu()
        drawn += int(valid.sum())
        unused += int((~valid).sum())
        for b in range(2):                                   # a frame changes iff it has a box
            assert bool((o["images"][b] != o["source"][b]).any()) == bool(valid[b * PIPE_K:(b + 1) * PIPE_K].any())
    print(f"overlay pipeline: conf {PIPE_CONF}: {drawn} boxes drawn, {unused} slots unused")
    assert drawn >= 1 and unused >= 1
    two = _run_pipeline("yolo_overlay_gpu.json", 2)
    for a, b in zip(one, two):
        for key in ("source", "images", "det", "count"):
            assert torch.equal(a[key], b[key]), key


def test_detector_only_pipeline_matches_direct_call(native):
    from aiko_services_amd.models.yolov8 import YOLOv8
    from aiko_services_amd.ops.overlay import draw_detections
    outs = _run_pipeline("yolo_overlay_detector_gpu.json", 1, frames=2)
    yolo = YOLOv8(scale="n", seed=0, device="cuda", conf=PIPE_CONF)
    names, font, palette, gw = _element_tables(80)
    for o in outs:
        det, count = yolo.detect(o["source"])
        direct = draw_detections(o["source"], det, count, PIPE_K, names.cuda(), font.cuda(), palette.cuda(),
                                 glyph_width=gw)
        torch.cuda.synchronize()
        assert torch.equal(o["det"], det) and torch.equal(o["count"], count)
        assert (count >= 1).any() and (direct != o["source"]).any()
        assert torch.equal(o["images"], direct)
