"""track_detections at the YOLO bench batch against the host round trip it replaces
(profiles/track.md).

B camera rows, K boxes considered per frame, T track slots per row, ``max_det`` rows per frame.  A
seeded scene of ``--frames`` instants: per row up to 1.5 K objects that drift, each present for a
stretch of the cycle; the detector's rows are the present objects in score order.  Measures

* the kernel: device events around ``--iters`` back-to-back steps (two state sets, ping-pong,
  cycling through the frames) after a warm-up — as eager calls, and as replays of a hipGraph that
  holds one cycle, which leaves the per-call enqueue out;
* a device copy of the same number of bytes (what one step reads and writes), timed the same way;
* the host path: rows and counts to pinned memory, the event wait, the same greedy tracker in
  numpy over all rows, the labels back to the device; host clock around each step, ending in a
  synchronise.

Usage:  python scripts/track_bench.py [--batch 192] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_scene(B, K, max_det, frames, seed):
    """[(det [B, max_det, 6], count [B])] * frames, on the CPU."""
    rng = np.random.default_rng(seed)
    N = K + K // 2
    w, h = rng.uniform(16, 160, (B, N)), rng.uniform(16, 120, (B, N))
    x0, y0 = rng.uniform(0, 640 - 160, (B, N)), rng.uniform(0, 480 - 120, (B, N))
    vx, vy = rng.uniform(-4, 4, (B, N)), rng.uniform(-4, 4, (B, N))
    score = rng.uniform(0.25, 0.95, (B, N))
    cls = rng.integers(0, 80, (B, N)).astype(np.float64)
    start, length = rng.integers(0, frames, (B, N)), rng.integers(2, frames + 1, (B, N))
    out = []
    for f in range(frames):
        present = ((f - start) % frames) < length
        s = np.where(present, score + rng.uniform(-0.02, 0.02, (B, N)), -1.0)
        order = np.argsort(-s, axis=1, kind="stable")
        x1, y1 = x0 + vx * f, y0 + vy * f
        rows = np.stack([x1, y1, x1 + w, y1 + h, s, cls], -1)
        rows = np.take_along_axis(rows, order[..., None], 1)
        det = np.zeros((B, max_det, 6), np.float32)
        n = min(N, max_det)
        det[:, :n] = rows[:, :n]
        out.append((torch.from_numpy(det), torch.from_numpy(present.sum(1).clip(max=max_det).astype(np.int32))))
    return out


class HostTracker:
    """The rules of ops/track.py in numpy, a row at a time: what a pipeline without the kernel
    runs between the detector and the overlay."""

    def __init__(self, B, T, iou, max_age, label_mod):
        self.boxes = np.zeros((B, T, 4), np.float32)
        self.meta = np.zeros((B, T, 4), np.int64)
        self.issued = np.zeros(B, np.int64)
        self.thr, self.max_age, self.label_mod = float(np.float32(iou)), max_age, label_mod

    def step(self, det, count, K):
        B = det.shape[0]
        ids = np.zeros((B, K), np.int32)
        for b in range(B):
            n = min(max(int(count[b]), 0), K)
            d = det[b, :n]
            valid = np.isfinite(d[:, :4]).all(1)
            meta, boxes = self.meta[b], self.boxes[b]
            live = meta[:, 0] != 0
            a = boxes[:, None, :]
            iw = np.maximum(np.minimum(a[..., 2], d[None, :, 2]) - np.maximum(a[..., 0], d[None, :, 0]), 0)
            ih = np.maximum(np.minimum(a[..., 3], d[None, :, 3]) - np.maximum(a[..., 1], d[None, :, 1]), 0)
            inter = iw * ih
            area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
            area_b = (d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])
            union = (area_a + area_b[None, :]) - inter
            i64, u64 = inter.astype(np.float64), union.astype(np.float64)
            ok = live[:, None] & valid[None, :] & (meta[:, 1:2] == d[None, :, 5].astype(np.int64)) & \
                (inter > 0) & (union > 0) & (i64 >= self.thr * u64)
            tt, dd = np.nonzero(ok)
            order = np.argsort(-(i64[tt, dd] / u64[tt, dd]), kind="stable")
            t_used, d_used = np.zeros(len(meta), bool), np.zeros(n, bool)
            det_track = np.full(n, -1)
            for j in order:
                t, i = tt[j], dd[j]
                if not t_used[t] and not d_used[i]:
                    t_used[t] = d_used[i] = True
                    det_track[i] = t
                    boxes[t] = d[i, :4]
                    meta[t, 2] += 1
                    meta[t, 3] = 0
            lost = live & ~t_used
            meta[lost, 3] += 1
            dead = lost & (meta[:, 3] > self.max_age)
            meta[dead] = 0
            boxes[dead] = 0
            free = np.nonzero(meta[:, 0] == 0)[0]
            born = np.nonzero(valid & ~d_used & (d[:, 4] >= 0.0))[0][:len(free)]
            for t, i in zip(free, born):
                self.issued[b] += 1
                boxes[t] = d[i, :4]
                meta[t] = (self.issued[b], int(d[i, 5]), 1, 0)
                det_track[i] = t
            hit = det_track >= 0
            ids[b, :n][hit] = meta[det_track[hit], 0]
        return ids


def timed(fn, iters, windows=3):
    out = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(iters):
            fn(i)
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / iters)
    return out


def measure(B, K, T, max_det, frames, iters, host_steps, seed, iou=0.3, max_age=30, label_mod=1000):
    from aiko_services_amd.ops.track import new_state, track_detections
    scene = make_scene(B, K, max_det, frames, seed)
    dev = [(d.cuda(), c.cuda()) for d, c in scene]
    states = [new_state(B, T, "cuda"), new_state(B, T, "cuda")]
    outs = [torch.empty(B * K, dtype=torch.int32, device="cuda") for _ in range(3)]

    def step(i):
        det, count = dev[i % frames]
        track_detections(det, count, states[i % 2], K, iou=iou, max_age=max_age, label_mod=label_mod,
                         state_out=states[(i + 1) % 2], ids=outs[0], hits=outs[1], labels=outs[2])

    # the ids of the first cycle, for the comparison with the host tracker
    kernel_ids = []
    for i in range(frames):
        step(i)
        kernel_ids.append(outs[0].cpu().view(B, K).numpy().copy())
    live = int((states[frames % 2].meta[:, :, 0] != 0).sum())
    for i in range(frames, frames + 20):
        step(i)
    torch.cuda.synchronize()
    kernel = timed(lambda i: step(frames + i), iters)       # frames is even: the ping-pong goes on
    # the same steps without the per-call enqueue: one cycle captured in a hipGraph, replayed
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(frames):
            step(i)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    replay = [v / frames for v in timed(lambda i: graph.replay(), max(iters // frames, 1))]

    # one step reads the K rows, the count and the state and writes the state and three outputs
    nbytes = B * (K * 24 + 4 + 2 * (T * 32 + 4) + 3 * K * 4)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(20):
        dst.copy_(src)
    copy = timed(lambda i: dst.copy_(src), iters)

    host = HostTracker(B, T, iou, max_age, label_mod)
    pin_det = torch.empty(B, K, 6, dtype=torch.float32, pin_memory=True)
    pin_count = torch.empty(B, dtype=torch.int32, pin_memory=True)
    pin_labels = torch.empty(B * K, dtype=torch.int32, pin_memory=True)
    labels_dev = torch.empty(B * K, dtype=torch.int32, device="cuda")
    parts = {"d2h_wait_us": [], "numpy_us": [], "h2d_us": [], "total_us": []}
    mismatch = 0
    for i in range(host_steps):
        det, count = dev[i % frames]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pin_det.copy_(det[:, :K], non_blocking=True)
        pin_count.copy_(count, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        t1 = time.perf_counter()
        ids = host.step(pin_det.numpy(), pin_count.numpy(), K)
        pin_labels.copy_(torch.from_numpy(np.where(ids > 0, ids % label_mod, -1).astype(np.int32).reshape(-1)))
        t2 = time.perf_counter()
        labels_dev.copy_(pin_labels, non_blocking=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if i < frames:
            mismatch += int((ids != kernel_ids[i]).sum())
        if i >= 2:                                          # the first steps warm the host path up
            for key, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                parts[key].append(v * 1e6)
    res = {"shape": {"B": B, "K": K, "T": T, "max_det": max_det, "frames": frames},
           "boxes_per_frame": round(float(np.mean([c.float().mean() for _, c in scene])), 2),
           "live_tracks_after_cycle": live,
           "kernel_us": round(min(kernel), 2), "kernel_us_windows": [round(v, 2) for v in kernel],
           "graph_step_us": round(min(replay), 2), "graph_step_us_windows": [round(v, 2) for v in replay],
           "bytes_per_step": nbytes, "copy_us": round(min(copy), 2), "copy_us_windows": [round(v, 2) for v in copy],
           "host_steps_timed": len(parts["total_us"]),
           **{"host_" + k: round(float(np.median(v)), 1) for k, v in parts.items()},
           "host_total_us_min": round(min(parts["total_us"]), 1),
           "ratio_host_over_kernel": round(float(np.median(parts["total_us"])) / min(kernel), 1),
           "ids_differing_from_host_tracker": mismatch}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[192, 8])
    ap.add_argument("--rois", type=int, default=16)
    ap.add_argument("--tracks", type=int, default=32)
    ap.add_argument("--max-det", type=int, default=300)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--host-steps", type=int, default=34)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.frames % 2:
        raise SystemExit("track_bench: an even --frames keeps the two state sets in step with the cycle")
    if not torch.cuda.is_available():
        raise SystemExit("track_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd.ops import require_native
    require_native()
    lines = []
    for B in a.batch:
        lines.append(json.dumps(measure(B, a.rois, a.tracks, a.max_det, a.frames, a.iters, a.host_steps, a.seed)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
