"""warp_quads at the marker pipeline's shape against a plain copy, roi_crop and the host path it
replaces, and FrameWarp's whole-frame views against a copy of the frames (profiles/warp.md).

B frames of H x W noise, K quads each (seeded convex quads of 60..240 pixels a side, turned and
foreshortened, all used), S x S patches.  Measures, each as device events around ``--iters``
back-to-back calls after a warm-up, three windows:

* ``warp_quads``;
* a device copy of as many bytes as it writes (``patches.copy_``);
* ``roi_crop`` at the same K and size on the quads' bounding boxes;
* ``warp_quads`` with one whole-frame quad per frame (K = 1, H x W out): ``rot180`` and a keystone
  quad, and a device copy of the frames;

and, on a host clock, ``warp_quads_ref`` (numpy, one core) on the first ``--ref-frames`` frames, the
path a pipeline without the kernel would take after copying frames and quads to the host; its patches
must equal the kernel's.

Usage:  python scripts/warp_bench.py [--out FILE.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_quads(B, K, H, W, seed):
    """int32 [B, K, 4, 2]: squares of 60..240 pixels turned by any angle, one side shortened to 0.6..1
    of its length, centred so that most of the quad is inside the frame."""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, K, 4, 2), np.int32)
    for b in range(B):
        for i in range(K):
            side, t, squeeze = rng.uniform(60, 240), rng.uniform(0, 2 * math.pi), rng.uniform(0.6, 1.0)
            cx, cy = rng.uniform(side / 2, W - side / 2), rng.uniform(side / 2, H - side / 2)
            h = side / 2
            for n, (x, y) in enumerate(((-h, -h), (h, -h * squeeze), (h, h * squeeze), (-h, h))):
                out[b, i, n] = (round(cx + math.cos(t) * x - math.sin(t) * y), round(cy + math.sin(t) * x + math.cos(t) * y))
    return torch.from_numpy(out)


def timed(fn, iters, windows=3, warmup=10):
    """Microseconds per call: the windows, each device events around ``iters`` calls."""
    for _ in range(warmup):
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
        runs.append(round(t0.elapsed_time(t1) * 1e3 / iters, 2))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--quads", type=int, default=4)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--ref-frames", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("warp_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd.ops import require_native
    from aiko_services_amd.ops.reference import warp_quads_ref
    from aiko_services_amd.ops.roi import roi_crop
    from aiko_services_amd.ops.warp import view_quad, warp_quads
    require_native()
    B, K, S, H, W = a.batch, a.quads, a.size, a.height, a.width
    g = torch.Generator().manual_seed(a.seed)
    frames_h = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    quads_h = make_quads(B, K, H, W, a.seed)
    count_h = torch.full((B,), K, dtype=torch.int32)
    frames, quads, count = frames_h.cuda(), quads_h.cuda(), count_h.cuda()
    patches = torch.empty(B * K, S, S, 3, dtype=torch.uint8, device="cuda")
    valid = torch.empty(B * K, dtype=torch.int32, device="cuda")
    spare = torch.empty_like(patches)

    warp = timed(lambda: warp_quads(frames, quads, count, K, (S, S), 0, "centre", patches=patches, valid=valid), a.iters)
    copy = timed(lambda: spare.copy_(patches), a.iters)
    # roi_crop on the bounding boxes of the same quads
    q = quads.float()
    det = torch.zeros(B, K, 6, device="cuda")
    det[..., 0], det[..., 1] = q[..., 0].amin(2).clamp(min=0), q[..., 1].amin(2).clamp(min=0)
    det[..., 2], det[..., 3] = (q[..., 0].amax(2) + 1).clamp(max=W), (q[..., 1].amax(2) + 1).clamp(max=H)
    det[..., 4] = 1.0
    crops = torch.empty_like(patches)
    rois = torch.empty(B * K, 4, dtype=torch.int32, device="cuda")
    crop = timed(lambda: roi_crop(frames, det, count, K, (S, S), 0.0, crops=crops, rois=rois), a.iters)

    # the host path: numpy on one core, a few frames; the patches must be the kernel's
    n = min(a.ref_frames, B)
    warp_quads_ref(frames_h[:1], quads_h[:1], count_h[:1], K, (S, S))           # warm-up
    t = time.perf_counter()
    want = warp_quads_ref(frames_h[:n], quads_h[:n], count_h[:n], K, (S, S))
    ref_us = (time.perf_counter() - t) * 1e6
    same = bool(torch.equal(patches[:n * K].cpu(), want[0]) and torch.equal(valid[:n * K].cpu(), want[1]))

    # whole frames: one quad per frame
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
    ok = torch.empty(B, dtype=torch.int32, device="cuda")
    ones = torch.ones(B, dtype=torch.int32, device="cuda")
    views = {"rot180": view_quad("rot180", H, W)[0],
             "keystone": [(W // 10, 0), (W - W // 10, 0), (W, H), (0, H)]}
    frame_us = {}
    for name, quad in views.items():
        fq = torch.tensor(quad, dtype=torch.int32).expand(B, 1, 4, 2).contiguous().cuda()
        frame_us[name] = timed(lambda: warp_quads(frames, fq, ones, 1, (H, W), 0, "edge", patches=out, valid=ok), a.iters)
        if name == "rot180":
            same = same and bool(torch.equal(out, frames.flip(1, 2)))
    frame_copy = timed(lambda: out.copy_(frames), a.iters)

    written = patches.numel() + valid.numel() * 4
    best = min(warp)
    res = {"shape": {"B": B, "H": H, "W": W, "K": K, "size": S}, "slots": B * K, "iters": a.iters,
           "warp_quads_us": warp, "copy_patches_us": copy, "roi_crop_us": crop,
           "bytes_written": written, "write_TBps": round(written / best / 1e6, 3),
           "pixels_per_us": round(B * K * S * S / best, 1),
           "ratio_warp_over_copy": round(best / min(copy), 2), "ratio_warp_over_roi_crop": round(best / min(crop), 2),
           "ref_frames": n, "ref_us": round(ref_us, 1), "ref_us_per_patch": round(ref_us / (n * K), 1),
           "ref_us_all_slots_one_core": round(ref_us / (n * K) * B * K, 1),
           "ratio_ref_over_warp": round(ref_us / (n * K) * B * K / best, 1),
           "frame_warp_us": frame_us, "copy_frames_us": frame_copy,
           "ratio_rot180_over_copy": round(min(frame_us["rot180"]) / min(frame_copy), 2),
           "ratio_keystone_over_copy": round(min(frame_us["keystone"]) / min(frame_copy), 2),
           "equal_to_reference": same}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("warp_bench: the kernel's patches differ from the reference")


if __name__ == "__main__":
    main()
