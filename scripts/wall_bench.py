"""frame_wall at the YOLO bench shape against a plain copy of the same frames, against resize_u8 and
against the host path it replaces (profiles/wall.md).

B frames of H x W seeded noise; two walls with the element's default tile: 4 x 4 on ceil(B / 16)
pages (tiles of H // 4 x W // 4) and 14 x 14 on one page (tiles of H // 14 x W // 14, the first 196
cameras or all of them).  Per wall, on the same tensors and in the same run:

* (a) frame_wall in index order with ring and labels on (every camera scores), (b) the same wall
  plain (no score, no ring, no label), (c) a score-ordered wall in which 16 of the B cameras
  reach ``min_score``, (d) the selection launch alone in score order, (e) the composition alone;
* (f) ``out.copy_(frames)`` of all B frames: the read (a) cannot beat, plus a write of the same size
  that the wall does not have; (g) ``resize_u8`` of all B frames to the tile size, for scale only:
  it is bilinear and reads four pixels per output pixel, not the whole footprint;
* all of them timed by device events around ``--iters`` back-to-back calls after a warm-up of 10, in
  ``--windows`` windows; the windows of the variants alternate (one window of each, then the next
  window of each), so that a drift of the clock meets all of them alike; median and spread reported;
* (h) once per wall the host path: ``frames.cpu()``, then a Pillow ``BOX`` resize per camera and a
  paste into the page; host clock around the whole thing;
* checked in the same run against ``frame_wall_ref``: the top two tile rows of the first page of
  (a) and (b), and the whole of (c);
* computed here from the shapes, not measured: the bytes (a) has to read and write.

Usage:  python scripts/wall_bench.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_together(fns, iters, windows):
    """{name: microseconds per call}: device events around ``iters`` back-to-back calls per window,
    the windows of the variants alternating; 10 warm-up calls each first."""
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    runs = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            runs[name].append(t0.elapsed_time(t1) * 1e3 / iters)
    return {name: {"median_us": round(statistics.median(r), 2), "min_us": round(min(r), 2),
                   "max_us": round(max(r), 2)} for name, r in runs.items()}


def host_path(frames, rows, cols, tile, pages, limit=None):
    """All frames to the host, then a Pillow BOX resize per camera pasted into its page."""
    import numpy as np
    from PIL import Image
    th, tw = tile
    frames_h = frames.cpu().numpy()                              # the sync
    n = frames_h.shape[0] if limit is None else limit
    wall = np.zeros((pages, rows * th, cols * tw, 3), np.uint8)
    for cam in range(min(n, pages * rows * cols)):
        p, t = divmod(cam, rows * cols)
        small = np.asarray(Image.fromarray(frames_h[cam]).resize((tw, th), Image.BOX))
        wall[p, (t // cols) * th:(t // cols + 1) * th, (t % cols) * tw:(t % cols + 1) * tw] = small
    return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-host", action="store_true", help="leave (h), the host path, out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wall_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd.ops import require_native
    from aiko_services_amd.ops.reference import frame_wall_ref
    from aiko_services_amd.ops.vision import resize_u8
    from aiko_services_amd.ops.wall import default_tile, frame_wall, wall_shape
    require_native()
    B, H, W = a.batch, a.height, a.width
    g = torch.Generator().manual_seed(a.seed)
    frames_h = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    frames = frames_h.cuda()
    every = torch.ones(B, dtype=torch.int32)                     # every camera scores: every tile ringed
    few_h = torch.zeros(B, dtype=torch.int32)                    # 16 cameras score, spread over the batch
    few_h[torch.randperm(B, generator=g)[:16]] = torch.randint(1, 50, (16,), generator=g).int()
    every_d, few_d = every.cuda(), few_h.cuda()
    copy = torch.empty_like(frames)
    walls = []
    for rows, cols in ((4, 4), (14, 14)):
        N = rows * cols
        pages = -(-B // N) if N < B else 1
        tile = default_tile(H, W, rows, cols)
        shown = min(B, pages * N)
        deco = dict(ring=2, label_scale=1)
        kw = dict(rows=rows, cols=cols, tile=tile)
        out = torch.empty(pages, *wall_shape(rows, cols, tile), 3, dtype=torch.uint8, device="cuda")
        source = torch.empty(pages, N, dtype=torch.int32, device="cuda")
        small = torch.empty(B, tile[0], tile[1], 3, dtype=torch.uint8, device="cuda")
        fns = {
            "a_wall": lambda: frame_wall(frames, every_d, out=out, source=source, **kw, **deco),
            "b_plain": lambda: frame_wall(frames, out=out, source=source, **kw),
            "c_score16": lambda: frame_wall(frames, few_d, order="score", out=out, source=source, **kw, **deco),
            "d_select": lambda: frame_wall(frames, few_d, order="score", out=out, source=source, passes=1, **kw),
            "f_copy": lambda: copy.copy_(frames),
            "g_resize_u8": lambda: resize_u8(frames, tile, small),
        }
        frame_wall(frames, every_d, out=out, source=source, **kw, **deco)       # the source (e) reads
        index_source = source.clone()
        fns["e_compose"] = lambda: frame_wall(frames, every_d, out=out, source=index_source, passes=2, **kw, **deco)
        t = timed_together(fns, a.iters, a.windows)
        check = {}
        n_ref = min(B, 2 * cols)                                 # index order: the top two tile rows of page 0
        for name, score, more in (("a_wall", every, deco), ("b_plain", None, {})):
            wall, src = frame_wall(frames, None if score is None else score.cuda(), pages=pages, **kw, **more)
            ref_wall, ref_src = frame_wall_ref(frames_h[:n_ref], None if score is None else score[:n_ref], **kw, **more)
            torch.cuda.synchronize()
            check[name] = bool(torch.equal(wall[0, :2 * tile[0]].cpu(), ref_wall[0, :2 * tile[0]])) and \
                bool(torch.equal(src[0, :n_ref].cpu(), ref_src[0, :n_ref]))
        wall, src = frame_wall(frames, few_d, order="score", pages=pages, **kw, **deco)
        ref_wall, ref_src = frame_wall_ref(frames_h, few_h, order="score", pages=pages, **kw, **deco)   # 16 tiles
        torch.cuda.synchronize()
        check["c_score16"] = bool(torch.equal(wall.cpu(), ref_wall)) and bool(torch.equal(src.cpu(), ref_src))
        host_us = pillow_max = None
        if not a.skip_host:
            host_path(frames, rows, cols, tile, pages, limit=2)  # warms Pillow up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = host_path(frames, rows, cols, tile, pages)
            host_us = (time.perf_counter() - t0) * 1e6
            wall, _ = frame_wall(frames, pages=pages, **kw)
            pillow_max = int((torch.from_numpy(host).int() - wall.cpu().int()).abs().max())
        read_bytes, write_bytes = shown * H * W * 3, out.numel()
        us = t["a_wall"]["median_us"]
        walls.append({"grid": [rows, cols], "pages": pages, "tile": list(tile), "shown": shown, "us": t,
                      "a_over_f_copy": round(us / t["f_copy"]["median_us"], 3),
                      "a_over_g_resize": round(us / t["g_resize_u8"]["median_us"], 3),
                      "bytes_read_computed": read_bytes, "bytes_written_computed": write_bytes,
                      "GBps_a_read": round(read_bytes / us / 1e3, 1),
                      "h_host_us": None if host_us is None else round(host_us, 1),
                      "h_over_a": None if host_us is None else round(host_us / us, 1),
                      "max_difference_from_pillow_box": pillow_max, "checks": check})
    res = {"shape": {"B": B, "H": H, "W": W}, "iters": a.iters, "windows": a.windows, "walls": walls}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
