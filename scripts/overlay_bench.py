"""draw_detections at the YOLO bench shape against a plain copy and against the host path it
replaces (profiles/overlay.md).

B frames of H x W, ``max_det`` rows each, random boxes from a seed, at three fill levels: every
frame with 0, about 10 (uniform in 5..15) and ``max_det`` used rows.  Per level:

* (a) draw_detections, out of place; (b) in place; (c) ``out.copy_(frames)`` of the same tensors,
  the floor of (a): device events around ``--iters`` back-to-back calls after a warm-up, in
  ``--windows`` windows (median and spread reported);
* (d) the host path: ``det`` / ``count`` / ``frames`` to the host, then the drawing loop of
  ``ImageOverlay`` (one PIL rectangle and one PIL text per box) on the same boxes; host clock around
  the whole thing;
* the mean length of the culled row list per tile, computed here on the host from the same boxes by
  the kernel's rule (a row is kept iff its label or its outline has a pixel in the tile).

Usage:  python scripts/overlay_bench.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE_W, TILE_H = 128, 32       # OV_TW, OV_TH of overlay_ops.hip
CLASSES = 80


def make_scene(B, H, W, max_det, lo, hi, seed):
    """Frames, det rows (boxes 16 px .. half the frame, scores descending) and counts in [lo, hi]."""
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    count = torch.randint(lo, hi + 1, (B,), generator=g).to(torch.int32)
    n = max_det
    w = 16 + torch.rand(B, n, generator=g) * (W / 2 - 16)
    h = 16 + torch.rand(B, n, generator=g) * (H / 2 - 16)
    x1 = torch.rand(B, n, generator=g) * (W - w)
    y1 = torch.rand(B, n, generator=g) * (H - h)
    score = torch.rand(B, n, generator=g).sort(1, descending=True).values
    cls = torch.randint(0, CLASSES, (B, n), generator=g).float()
    rows = torch.stack([x1, y1, x1 + w, y1 + h, score, cls], -1)
    live = torch.arange(n)[None, :] < count[:, None]
    pad = torch.zeros(B, n, 6)
    pad[:, :, 5] = -1
    return frames, torch.where(live[..., None], rows, pad).contiguous(), count


def culled_per_tile(det, count, K, H, W, thickness, scale, name_len, gw, gh):
    """Mean and max number of rows a tile keeps, and the share of tiles that keep none."""
    from aiko_services_amd.ops.reference import roi_rects_ref
    B = det.shape[0]
    r = roi_rects_ref(det, count, K, (H, W), 0.0).view(B, K, 4).long()
    x0, y0, x1, y1 = r.unbind(-1)
    used = x1 > x0
    cls = det[:, :K, 5].long().clamp(0, CLASSES - 1)
    nch = name_len[cls] + 3                                    # name, space, two digits
    lw, lh = nch * gw * scale + 2 * scale, gh * scale + 2 * scale
    lx = torch.minimum(x0, W - lw).clamp(min=0)
    ly = torch.where(y0 - lh >= 0, y0 - lh, y0)
    lx1, ly1 = (lx + lw).clamp(max=W), (ly + lh).clamp(max=H)
    tx0 = torch.arange(0, W, TILE_W)
    ty0 = torch.arange(0, H, TILE_H)
    tx1, ty1 = (tx0 + TILE_W).clamp(max=W), (ty0 + TILE_H).clamp(max=H)
    e = lambda v: v[:, :, None, None]                          # noqa: E731  rows -> [B, K, 1, 1]
    X0, X1, Y0, Y1 = tx0[None, None, None, :], tx1[None, None, None, :], ty0[None, None, :, None], ty1[None, None, :, None]
    touch = lambda a0, b0, a1, b1: (e(a0) < X1) & (e(a1) > X0) & (e(b0) < Y1) & (e(b1) > Y0)  # noqa: E731
    t = thickness
    interior = (X0 >= e(x0) + t) & (X1 <= e(x1) - t) & (Y0 >= e(y0) + t) & (Y1 <= e(y1) - t)
    keep = ((touch(lx, ly, lx1, ly1) & e(nch > 0)) | (touch(x0, y0, x1, y1) & ~interior)) & e(used)
    per_tile = keep.sum(1).float()                             # [B, tiles y, tiles x]
    return float(per_tile.mean()), int(per_tile.max()), float((per_tile == 0).float().mean())


def host_path(frames, det, count, K, names, thickness, limit=None):
    """Rows and frames to the host, then ImageOverlay's loop: a PIL rectangle and text per box."""
    import numpy as np
    from PIL import Image, ImageDraw
    det_h, count_h, frames_h = det.cpu(), count.cpu(), frames.cpu().numpy()      # the sync
    if limit is not None:                                      # a warm-up on the first frames only
        frames_h = frames_h[:limit]
    color = (0, 255, 255)
    out = []
    for b in range(frames_h.shape[0]):
        pil = Image.fromarray(frames_h[b]).convert("RGB")
        draw = ImageDraw.Draw(pil)
        for x1, y1, x2, y2, conf, cls in det_h[b, :min(int(count_h[b]), K)].tolist():
            x, y, w, h = int(x1), int(y1), int(x2 - x1), int(y2 - y1)
            draw.rectangle([x, y, x + w, y + h], outline=color, width=thickness)
            ty = y - 12 if y > 14 else y + h + 2
            draw.text((x, ty), f"{names[int(cls)]}: {conf:0.2f}", fill=color)
        out.append(np.asarray(pil))
    return out


def timed(fn, iters, windows):
    """Microseconds per call: device events around ``iters`` back-to-back calls, per window."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        runs.append(t0.elapsed_time(t1) * 1e3 / iters)
    return {"median_us": round(statistics.median(runs), 2), "min_us": round(min(runs), 2),
            "max_us": round(max(runs), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--max-det", type=int, default=300)
    ap.add_argument("--thickness", type=int, default=2)
    ap.add_argument("--text-scale", type=int, default=1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-labels", action="store_true", help="outlines only: an empty name table, no score")
    ap.add_argument("--skip-host", action="store_true", help="leave (d), the host path, out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlay_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd.ops import require_native
    from aiko_services_amd.ops.overlay import default_font, default_palette, draw_detections, pack_names
    require_native()
    B, H, W, K = a.batch, a.height, a.width, a.max_det
    name_list = [f"class_{i}" for i in range(CLASSES)]
    font, gw = default_font()
    names, palette = pack_names(name_list, 16), default_palette(20)
    name_len = torch.tensor([len(n) for n in name_list])
    dn, df, dp = names.cuda(), font.cuda(), palette.cuda()
    kw = dict(thickness=a.thickness, text_scale=a.text_scale, glyph_width=gw)
    if a.no_labels:
        dn, name_len = dn[:0], name_len * 0 - 3
        kw["show_score"] = False
    levels = []
    for label, lo, hi in (("0", 0, 0), ("about 10", 5, 15), (str(K), K, K)):
        frames_h, det_h, count_h = make_scene(B, H, W, K, lo, hi, a.seed)
        frames, det, count = frames_h.cuda(), det_h.cuda(), count_h.cuda()
        out = torch.empty_like(frames)
        inplace = frames.clone()
        ta = timed(lambda: draw_detections(frames, det, count, K, dn, df, dp, out=out, **kw), a.iters, a.windows)
        tb = timed(lambda: draw_detections(inplace, det, count, K, dn, df, dp, out=inplace, **kw), a.iters, a.windows)
        tc = timed(lambda: out.copy_(frames), a.iters, a.windows)
        draw_detections(frames, det, count, K, dn, df, dp, out=out, **kw)
        torch.cuda.synchronize()
        same = bool(torch.equal(out, inplace))
        drawn = float((out != frames).any(-1).float().mean())
        host = []
        if not a.skip_host:
            host_path(frames, det, count, K, name_list, a.thickness, limit=2)   # warms PIL up
        for _ in range(0 if a.skip_host else a.host_reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            host_path(frames, det, count, K, name_list, a.thickness)
            host.append((time.perf_counter() - t) * 1e6)
        td = min(host) if host else float("nan")
        mean_list, max_list, empty = culled_per_tile(det_h, count_h, K, H, W, a.thickness, a.text_scale, name_len,
                                                     gw, font.shape[1])
        levels.append({"count": label, "boxes": int(count_h.sum()), "a_out_of_place": ta, "b_in_place": tb,
                       "c_copy": tc, "d_host_us": round(td, 1) if host else None, "d_host_us_reps": [round(h, 1) for h in host],
                       "a_over_c": round(ta["median_us"] / tc["median_us"], 3),
                       "d_over_a": round(td / ta["median_us"], 1) if host else None,
                       "GBps_a": round(2 * frames.numel() / ta["median_us"] / 1e3, 1),
                       "share_of_pixels_drawn": round(drawn, 4), "in_place_equals_out_of_place": same,
                       "mean_rows_per_tile": round(mean_list, 3), "max_rows_per_tile": max_list,
                       "share_of_empty_tiles": round(empty, 4)})
    res = {"shape": {"B": B, "H": H, "W": W, "max_det": K, "thickness": a.thickness, "text_scale": a.text_scale,
                     "tile": [TILE_W, TILE_H]},
           "labels": not a.no_labels, "iters": a.iters, "windows": a.windows, "levels": levels}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
