"""motion_detect at the YOLO bench shape: the cell pass against a plain copy of the same frames, the
region pass on three masks, and the whole step against the host path it replaces
(profiles/motion.md).

B frames of H x W uint8 noise; a "typical" step is a still camera with a few rectangles of other
noise pasted into every frame (``--blobs`` per frame, 2..6 cells a side at cell 16).  In one run:

* (a) the cell pass alone (``aiko_motion_cells`` of the built library, called directly) and (b)
  ``out.copy_(frames)`` on the same frames; then both again over ``--rotate`` distinct frame
  buffers taken in turn, whose total is past the 256 MB Infinity Cache;
* the region pass alone (``aiko_motion_regions``) on (c) an empty mask, (d) the typical mask and (e)
  a serpentine on the 1080p / cell 16 grid (68 x 120), B frames each;
* (f) the whole step, ``ops.motion.motion_detect`` with every output preallocated;
* all of them timed by device events around ``--iters`` back-to-back calls after a warm-up of 10, in
  ``--windows`` windows; the windows of the variants alternate; median and spread reported;
* (g) once, by the host clock: the frames to the host, the same rule in numpy (cell sums by
  ``np.add.reduceat``, components by ``scipy.ndimage.label`` where scipy is installed, by a
  breadth-first walk otherwise), the rows back to the device;
* checked in the same run: the two passes called directly equal the operator, the first two frames
  equal ``motion_detect_ref``, (g) equals the operator on every frame.

Usage:  python scripts/motion_bench.py [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KW = dict(cell=16, threshold=12, learn_shift=4, learn_moving=True, warmup=1, min_cells=2, max_det=16)
READ_ROOF_TBPS, COPY_ROOF_TBPS = 6.83, 5.67        # profiles/hbm_roof_r6.md, one stream


def passes():
    """``(cells_fn, regions_fn)`` launching the two passes of motion_ops.hip on the current stream."""
    import aiko_services_amd
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(aiko_services_amd.__file__)), "_C.so"))
    cells, regions = lib.aiko_motion_cells, lib.aiko_motion_regions
    cells.restype = regions.restype = ctypes.c_int
    cells.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 8 + [ctypes.c_void_p]
    regions.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 6 + [ctypes.c_void_p]

    def cells_fn(frames, state, state_out, mask, kw=KW):
        B, H, W, _ = frames.shape
        rc = cells(frames.data_ptr(), state.bg.data_ptr(), state.seen.data_ptr(), state_out.bg.data_ptr(),
                   state_out.seen.data_ptr(), mask.data_ptr(), B, H, W, kw["cell"], kw["threshold"], kw["learn_shift"],
                   int(kw["learn_moving"]), kw["warmup"], torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"aiko_motion_cells returned {rc}")

    def regions_fn(mask, hw, det, count, ncells, kw=KW):
        rc = regions(mask.data_ptr(), det.data_ptr(), count.data_ptr(), ncells.data_ptr(), mask.shape[0], hw[0], hw[1],
                     kw["cell"], kw["min_cells"], det.shape[1], torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"aiko_motion_regions returned {rc}")

    cells_fn.keep = lib
    return cells_fn, regions_fn


def make_frames(B, H, W, blobs, seed):
    """(still, moved): uint8 ``[B, H, W, 3]`` noise, and the same with ``blobs`` rectangles of other
    noise per frame, 2..6 cells of 16 pixels a side, on the cell grid."""
    g = torch.Generator().manual_seed(seed)
    still = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    moved = still.clone()
    gh, gw = H // 16, W // 16
    for b in range(B):
        for _ in range(blobs):
            h, w = (int(v) for v in torch.randint(2, 7, (2,), generator=g))
            y, x = int(torch.randint(0, gh - h + 1, (1,), generator=g)), int(torch.randint(0, gw - w + 1, (1,), generator=g))
            # a flat patch: far from the noise's cell mean of about 127
            moved[b, 16 * y:16 * (y + h), 16 * x:16 * (x + w)] = int(torch.randint(0, 64, (1,), generator=g))
    return still, moved


def serpentine(gh, gw):
    m = np.zeros((gh, gw), np.uint8)
    m[0::2] = 1
    for i, gy in enumerate(range(1, gh, 2)):
        m[gy, gw - 1 if i % 2 == 0 else 0] = 1
    return m


def host_regions(mask, H, W, kw):
    """Rule 6 and 7 of ops/motion.py on one uint8 ``[Gh, Gw]`` mask -> (rows fp32 [max_det, 6], count)."""
    cell, gw = kw["cell"], mask.shape[1]
    rows = np.zeros((kw["max_det"], 6), np.float32)
    try:
        from scipy import ndimage
        lab, n = ndimage.label(mask, structure=np.ones((3, 3), np.int8))
        comps = []
        for k, sl in enumerate(ndimage.find_objects(lab)):
            ys, xs = np.nonzero(lab[sl] == k + 1)
            first = int((ys * 10 ** 6 + xs).argmin())
            comps.append((len(ys), (sl[0].start + int(ys[first])) * gw + sl[1].start + int(xs[first]), sl[1].start,
                          sl[0].start, sl[1].stop - 1, sl[0].stop - 1))
    except ImportError:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        from motion_scenes import components
        comps = [(v[0], k, *v[1:]) for k, v in components(mask).items()]
    comps = sorted((c for c in comps if c[0] >= kw["min_cells"]), key=lambda c: (-c[0], c[1]))[:kw["max_det"]]
    for i, (area, _, cx0, cy0, cx1, cy1) in enumerate(comps):
        rows[i] = (cx0 * cell, cy0 * cell, min((cx1 + 1) * cell, W), min((cy1 + 1) * cell, H),
                   np.float32(area / ((cx1 - cx0 + 1) * (cy1 - cy0 + 1))), 0)
    return rows, len(comps)


def host_path(frames, bg, seen, kw, device):
    """The path the operator replaces: frames to the host, the rule in numpy, rows back to the device."""
    f = frames.cpu().numpy().astype(np.int32)                                # the sync
    B, H, W, _ = f.shape
    cell = kw["cell"]
    luma = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8
    ri, ci = np.arange(0, H, cell), np.arange(0, W, cell)
    S = np.add.reduceat(np.add.reduceat(luma, ri, 1), ci, 2).astype(np.int64)
    n = (np.minimum(cell, H - ri)[:, None] * np.minimum(cell, W - ci)[None, :])[None]
    cur = (32 * S + n) // (2 * n)
    s = np.maximum(seen, 0)[:, None, None]
    d = cur - bg
    moving = (s >= kw["warmup"]) & (np.abs(d) > 16 * kw["threshold"])
    half = (1 << (kw["learn_shift"] - 1)) if kw["learn_shift"] else 0
    learnt = bg + ((d + half) >> kw["learn_shift"])
    keep = moving & (not kw["learn_moving"])
    new_bg = np.where(s == 0, cur, np.where(keep, bg, learnt))
    det = np.zeros((B, kw["max_det"], 6), np.float32)
    count = np.zeros(B, np.int32)
    mask = moving.astype(np.uint8)
    for b in range(B):
        det[b], count[b] = host_regions(mask[b], H, W, kw)
    out = (torch.from_numpy(det).to(device), torch.from_numpy(count).to(device))
    torch.cuda.synchronize()
    return out, mask, new_bg, np.minimum(np.maximum(seen, 0) + 1, 2 ** 31 - 1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--blobs", type=int, default=4)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-host", action="store_true", help="leave (g), the host path, out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("motion_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd.ops import require_native
    from aiko_services_amd.ops.motion import MotionState, grid_shape, motion_detect, new_state
    from aiko_services_amd.ops.reference import motion_detect_ref
    require_native()
    cells_fn, regions_fn = passes()
    B, H, W = a.batch, a.height, a.width
    gh, gw = grid_shape(H, W, KW["cell"])
    dev = "cuda"
    still_h, moved_h = make_frames(B, H, W, a.blobs, a.seed)
    still, moved = still_h.to(dev), moved_h.to(dev)

    def outputs(g0, g1):
        return (torch.empty(B, KW["max_det"], 6, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                torch.empty(B, g0, g1, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev))

    # the state after the still frame: what every timed step starts from
    learnt = motion_detect(still, new_state(B, H, W, KW["cell"], dev), **KW)[4]
    state_out = new_state(B, H, W, KW["cell"], dev)
    det, count, mask, ncells = outputs(gh, gw)
    motion_detect(moved, learnt, state_out=state_out, det=det, count=count, mask=mask, cells=ncells, **KW)
    torch.cuda.synchronize()
    typical = mask.clone()
    checks = {}
    # the passes called directly give what the operator gave
    d2, c2, m2, n2 = outputs(gh, gw)
    s2 = new_state(B, H, W, KW["cell"], dev)
    cells_fn(moved, learnt, s2, m2)
    regions_fn(m2, (H, W), d2, c2, n2)
    torch.cuda.synchronize()
    checks["passes_equal_operator"] = all(bool(torch.equal(x, y)) for x, y in
                                          zip((d2, c2, m2, n2, *s2), (det, count, mask, ncells, *state_out)))
    want = motion_detect_ref(moved_h[:2], MotionState(learnt.bg[:2].cpu(), learnt.seen[:2].cpu()), **KW)
    checks["first_frames_equal_reference"] = all(bool(torch.equal(x[:2].cpu(), y)) for x, y in
                                                 zip((det, count, mask, ncells, *state_out), (*want[:4], *want[4])))

    # (a), (b): the cell pass and a copy, on one buffer and over buffers past the Infinity Cache
    copy_out = torch.empty_like(moved)
    ring = [moved] + [torch.randint(0, 256, moved.shape, dtype=torch.uint8, device=dev) for _ in range(a.rotate - 1)]
    turn = {"cells": 0, "copy": 0}

    def rotating(name, fn):
        def call():
            turn[name] = (turn[name] + 1) % len(ring)
            fn(ring[turn[name]])
        return call

    fns = {"a_cells": lambda: cells_fn(moved, learnt, s2, m2), "b_copy": lambda: copy_out.copy_(moved),
           "a_cells_rotating": rotating("cells", lambda f: cells_fn(f, learnt, s2, m2)),
           "b_copy_rotating": rotating("copy", lambda f: copy_out.copy_(f))}
    # (c), (d), (e): the region pass
    empty = torch.zeros_like(typical)
    g0, g1 = grid_shape(1080, 1920, 16)
    worst = torch.from_numpy(serpentine(g0, g1))[None].repeat(B, 1, 1).contiguous().to(dev)
    rw = outputs(g0, g1)
    fns["c_regions_empty"] = lambda: regions_fn(empty, (H, W), d2, c2, n2)
    fns["d_regions_typical"] = lambda: regions_fn(typical, (H, W), d2, c2, n2)
    fns["e_regions_serpentine_1080p"] = lambda: regions_fn(worst, (1080, 1920), rw[0], rw[1], rw[3])
    # (f): the whole step
    fns["f_motion_detect"] = lambda: motion_detect(moved, learnt, state_out=state_out, det=det, count=count,
                                                   mask=mask, cells=ncells, **KW)
    t = timed_together(fns, a.iters, a.windows)
    regions_fn(worst, (1080, 1920), rw[0], rw[1], rw[3])
    torch.cuda.synchronize()
    rows, n = host_regions(worst[0].cpu().numpy(), 1080, 1920, KW)
    checks["serpentine_equals_host"] = bool(torch.equal(rw[0][0].cpu(), torch.from_numpy(rows))) and \
        int(rw[1][0]) == n == 1 and int(rw[3][0]) == int(worst[0].sum())

    host_us = None
    if not a.skip_host:
        bg_h, seen_h = learnt.bg.cpu().numpy().astype(np.int64), learnt.seen.cpu().numpy().astype(np.int64)
        host_path(moved[:2], bg_h[:2], seen_h[:2], KW, dev)                 # warms numpy up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        (hd, hc), hm, hbg, hseen = host_path(moved, bg_h, seen_h, KW, dev)
        host_us = (time.perf_counter() - t0) * 1e6
        motion_detect(moved, learnt, state_out=state_out, det=det, count=count, mask=mask, cells=ncells, **KW)
        torch.cuda.synchronize()
        checks["host_equals_operator"] = bool(torch.equal(hd, det)) and bool(torch.equal(hc, count)) and \
            bool((torch.from_numpy(hm) == mask.cpu()).all()) and \
            bool((torch.from_numpy(hbg) == state_out.bg.cpu()).all()) and \
            bool((torch.from_numpy(hseen) == state_out.seen.cpu()).all())

    nbytes = moved.numel()
    a_us, b_us = t["a_cells"]["median_us"], t["b_copy"]["median_us"]
    ar_us, br_us = t["a_cells_rotating"]["median_us"], t["b_copy_rotating"]["median_us"]
    res = {"shape": {"B": B, "H": H, "W": W, "grid": [gh, gw], **KW}, "iters": a.iters, "windows": a.windows,
           "frame_bytes": nbytes, "rotating_bytes": nbytes * len(ring), "us": t,
           "a_over_b": round(a_us / b_us, 3), "a_over_b_rotating": round(ar_us / br_us, 3),
           "a_read_TBps": round(nbytes / a_us / 1e6, 2), "a_rotating_read_TBps": round(nbytes / ar_us / 1e6, 2),
           "b_copy_TBps": round(2 * nbytes / b_us / 1e6, 2), "b_rotating_copy_TBps": round(2 * nbytes / br_us / 1e6, 2),
           "a_rotating_share_of_read_roof": round(nbytes / ar_us / 1e6 / READ_ROOF_TBPS, 3),
           "b_rotating_share_of_copy_roof": round(2 * nbytes / br_us / 1e6 / COPY_ROOF_TBPS, 3),
           "typical": {"moving_cells_per_frame": round(float(ncells.float().mean()), 2),
                       "rows_per_frame": round(float(count.float().mean()), 2)},
           "serpentine_cells": int(worst[0].sum()),
           "g_host_us": None if host_us is None else round(host_us, 1),
           "g_over_f": None if host_us is None else round(host_us / t["f_motion_detect"]["median_us"], 1),
           "checks": checks}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
