"""roi_crop at the YOLO bench shape against the host loop it replaces (profiles/roi_crop.md).

B frames of H x W, K ROI slots each, S x S crops; per-frame counts and boxes from a seed (counts
uniform in [0, 2K): about half the frames have fewer than K boxes).  Measures

* roi_crop: device events around ``--iters`` back-to-back calls after a warm-up;
* the loop: ``det.cpu()``, ``count.cpu()``, the rects on the host, then one ``resize_u8`` per used
  slot into the same crops buffer; host clock around the whole thing, ending in a synchronise;
* the bytes roi_crop writes (crops + rois) per second.

Usage:  python scripts/roi_crop_bench.py [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WRITE_ROOF_TBS = 5.41          # profiles/hbm_roof_r6.md: write-only, one stream


def make_scene(B, H, W, K, max_det, seed, device):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    count = torch.randint(0, 2 * K, (B,), generator=g).to(torch.int32)
    det = torch.zeros(B, max_det, 6)
    det[:, :, 5] = -1
    n = 2 * K
    w = 16 + torch.rand(B, n, generator=g) * (W / 2 - 16)
    h = 16 + torch.rand(B, n, generator=g) * (H / 2 - 16)
    x1 = torch.rand(B, n, generator=g) * (W - w)
    y1 = torch.rand(B, n, generator=g) * (H - h)
    score = torch.rand(B, n, generator=g).sort(1, descending=True).values
    cls = torch.randint(0, 80, (B, n), generator=g).float()
    rows = torch.stack([x1, y1, x1 + w, y1 + h, score, cls], -1)
    live = torch.arange(n)[None, :] < count[:, None]
    det[:, :n] = torch.where(live[..., None], rows, det[:, :n])
    return frames.to(device), det.to(device), count.to(device)


def host_loop(frames, det, count, K, size, margin, crops):
    """The cascade without roi_crop: rows to the host, one resize launch per box."""
    from aiko_services_amd.ops.reference import roi_rects_ref
    from aiko_services_amd.ops.vision import resize_u8
    det_h, count_h = det.cpu(), count.cpu()                      # the sync
    rois = roi_rects_ref(det_h, count_h, K, frames.shape[1:3], margin).tolist()
    launches = 0
    for slot, (x0, y0, x1, y1) in enumerate(rois):
        if x1 > x0:
            resize_u8(frames[slot // K, y0:y1, x0:x1][None], size, out=crops[slot:slot + 1])
            launches += 1
    return launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--rois", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--max-det", type=int, default=300)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--loop-reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("roi_crop_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd.ops import require_native
    from aiko_services_amd.ops.roi import roi_crop
    require_native()
    B, K, S = a.batch, a.rois, a.size
    frames, det, count = make_scene(B, a.height, a.width, K, a.max_det, a.seed, "cuda")
    crops = torch.empty(B * K, S, S, 3, dtype=torch.uint8, device="cuda")
    rois = torch.empty(B * K, 4, dtype=torch.int32, device="cuda")
    for _ in range(10):
        roi_crop(frames, det, count, K, (S, S), 0.0, crops=crops, rois=rois)
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):                                           # spread: three timed windows
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            roi_crop(frames, det, count, K, (S, S), 0.0, crops=crops, rois=rois)
        t1.record()
        torch.cuda.synchronize()
        runs.append(t0.elapsed_time(t1) * 1e3 / a.iters)
    fused_us = min(runs)
    fused = crops.clone()
    used = int((rois[:, 2] > rois[:, 0]).sum())

    loop_crops = torch.zeros_like(crops)
    launches = host_loop(frames, det, count, K, (S, S), 0.0, loop_crops)    # warm-up
    torch.cuda.synchronize()
    loop = []
    for _ in range(a.loop_reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        host_loop(frames, det, count, K, (S, S), 0.0, loop_crops)
        torch.cuda.synchronize()
        loop.append((time.perf_counter() - t) * 1e6)
    loop_us = min(loop)
    diff = int((fused.int() - loop_crops.int()).abs().max())

    written = crops.numel() + rois.numel() * 4
    res = {"shape": {"B": B, "H": a.height, "W": a.width, "K": K, "size": S, "max_det": a.max_det},
           "slots": B * K, "used_slots": used, "frames_below_K": int((count < K).sum()),
           "roi_crop_us": round(fused_us, 2), "roi_crop_us_windows": [round(r, 2) for r in runs],
           "loop_us": round(loop_us, 1), "loop_us_reps": [round(r, 1) for r in loop], "loop_launches": launches,
           "ratio_loop_over_fused": round(loop_us / fused_us, 1),
           "bytes_written": written, "write_TBps": round(written / fused_us / 1e6, 3),
           "share_of_write_roof": round(written / fused_us / 1e6 / WRITE_ROOF_TBS, 3),
           "max_abs_diff_fused_vs_loop": diff}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
