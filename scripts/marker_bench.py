"""detect_markers at the vision bench shape: each pass and the whole step against a plain copy of the
same frames, the region pass at three candidate loads, and the whole step against the host detector
it stands in for (profiles/marker.md).

B frames of H x W: white under a lighting ramp with +-6 levels of noise and ``--markers`` original
markers per frame at random angles ("typical"); the same with no marker ("blank") and with 32 small
markers ("full": ``max_cand`` candidates).  ``--rotate`` copies of the frames are taken in turn, so
that their total is past the 256 MB Infinity Cache.  In one run:

* the range pass, the mask pass and the region pass alone (the operator's ``passes`` bits; a pass
  alone works on what the earlier ones left in the workspace), the whole step, and
  ``out.copy_(frames)`` on the same frames;
* the region pass alone on the blank, the typical and the full frames;
* all timed by device events around ``--iters`` back-to-back calls after a warm-up of 5, in
  ``--windows`` windows; the windows of the variants alternate; median and spread reported;
* by the host clock: ``detect_markers_numpy`` over ``--host-frames`` of the typical frames on one
  core, and the upload of the frames from pinned memory;
* checked in the same run: the first two typical frames equal ``detect_markers_ref``, and every
  planted marker of every typical frame is found under its id.

Usage:  python scripts/marker_bench.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KW = dict(dictionary="original", cell=4, contrast=64, min_side=24, max_cand=32, max_det=16)
READ_ROOF_TBPS, COPY_ROOF_TBPS = 6.83, 5.67        # profiles/hbm_roof_r6.md, one stream


def make_frames(B, H, W, markers, seed, distinct=8):
    """(uint8 [B, H, W, 3], ids per frame): ``distinct`` different frames, repeated up to B."""
    import marker_scenes as S
    rng = np.random.default_rng(seed)
    frames, ids = [], []
    cols = 8 if markers > 4 else 2
    rows = -(-markers // cols) if markers else 0
    side = 35 if markers > 4 else 84
    for _ in range(distinct):
        gray = np.full((H, W), float(S.WHITE)) + rng.integers(-6, 7, (H, W))
        planted = []
        for k in range(markers):
            cx, cy = (k % cols + 0.5) * W / cols, (k // cols + 0.5) * H / rows
            marker_id = int(rng.integers(1, 1023))
            while marker_id in planted or marker_id in (0, 1023) or \
                    np.array_equal(S.module_grid("original", marker_id), np.rot90(S.module_grid("original", marker_id), 2)):
                marker_id = int(rng.integers(1, 1023))
            S.paint(gray, S.module_grid("original", marker_id), S.square(cx, cy, side, float(rng.uniform(0, 360))))
            planted.append(marker_id)
        frames.append(S.light(gray))
        ids.append(sorted(planted))
    reps = -(-B // distinct)
    return torch.stack(frames).repeat(reps, 1, 1, 1)[:B].contiguous(), (ids * reps)[:B]


def timed(fns, iters, windows):
    """{name: [ms per call, ...]}: ``windows`` windows of ``iters`` calls each, the variants alternating."""
    out = {name: [] for name in fns}
    for name, fn in fns.items():
        for i in range(5):
            fn(i)
    torch.cuda.synchronize()
    for w in range(windows):
        for name, fn in fns.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for i in range(iters):
                fn(i)
            end.record()
            end.synchronize()
            out[name].append(start.elapsed_time(end) / iters)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--markers", type=int, default=4)
    ap.add_argument("--rotate", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("marker_bench: a GPU is required")
    from aiko_services_amd.examples.aruco_marker.aruco import detect_markers_numpy
    from aiko_services_amd.ops import require_native
    from aiko_services_amd.ops.marker import DICTIONARIES, detect_markers, grid_shape, work_size
    from aiko_services_amd.ops.reference import detect_markers_ref
    require_native()
    B, H, W = a.batch, a.height, a.width
    gh, gw = grid_shape(H, W, KW["cell"])
    host = {"blank": make_frames(B, H, W, 0, 1), "typical": make_frames(B, H, W, a.markers, 2),
            "full": make_frames(B, H, W, 32, 3)}
    dev = {k: [v[0].cuda() for _ in range(a.rotate)] for k, v in host.items()}
    i32 = torch.int32
    out = dict(det=torch.empty(B, KW["max_det"], 6, device="cuda"), count=torch.empty(B, dtype=i32, device="cuda"),
               corners=torch.empty(B, KW["max_det"], 4, 2, dtype=i32, device="cuda"),
               ids=torch.empty(B, KW["max_det"], dtype=i32, device="cuda"), cands=torch.empty(B, dtype=i32, device="cuda"),
               mask=torch.empty(B, gh, gw, dtype=torch.uint8, device="cuda"),
               work=torch.empty(work_size(B, H, W), dtype=i32, device="cuda"))
    copy = torch.empty_like(dev["typical"][0])

    def run(frames, passes=7):
        torch.ops.aiko.marker_detect_out(frames, DICTIONARIES[KW["dictionary"]], KW["cell"], KW["contrast"],
                                         KW["min_side"], KW["max_cand"], passes, out["det"], out["count"],
                                         out["corners"], out["ids"], out["cands"], out["mask"], out["work"])

    # the checks first
    checks = {}
    det, count, corners, ids, cands, mask = detect_markers(dev["typical"][0], **KW)
    torch.cuda.synchronize()
    want = detect_markers_ref(host["typical"][0][:2], **KW)
    got = [t[:2].cpu() for t in (det, count, corners, ids, cands, mask)]
    checks["first_two_frames_equal_reference"] = all(torch.equal(g, w) for g, w in zip(got, want))
    found = [sorted(ids[b, :int(count[b])].tolist()) for b in range(B)]
    checks["every_planted_marker_found"] = found == host["typical"][1]
    for name in ("blank", "full"):
        c = detect_markers(dev[name][0], **{**KW, "max_det": 64 if name == "full" else 16})
        torch.cuda.synchronize()
        checks[f"{name}_cands"] = sorted(set(c[4].tolist()))
        checks[f"{name}_counts"] = sorted(set(c[1].tolist()))
    checks["typical_cands"] = sorted(set(cands.tolist()))
    print(json.dumps(checks))
    if not (checks["first_two_frames_equal_reference"] and checks["every_planted_marker_found"]):
        raise SystemExit("marker_bench: the device result is wrong")

    fns = {"copy": lambda i: copy.copy_(dev["typical"][i % a.rotate]),
           "range": lambda i: run(dev["typical"][i % a.rotate], 1),
           "mask": lambda i: run(dev["typical"][i % a.rotate], 2),
           "regions_typical": lambda i: run(dev["typical"][i % a.rotate], 4),
           "step": lambda i: run(dev["typical"][i % a.rotate], 7)}
    run(dev["typical"][0])
    times = timed(fns, a.iters, a.windows)
    for name in ("blank", "full"):                          # the region pass on its own mask and words
        run(dev[name][0])
        times.update(timed({f"regions_{name}": lambda i, f=dev[name][0]: run(f, 4),
                            f"step_{name}": lambda i, f=dev[name]: run(f[i % a.rotate], 7)}, a.iters, a.windows))

    # the host detector on one core, and the upload
    torch.set_num_threads(1)
    n = min(a.host_frames, B)
    frames_np = host["typical"][0][:n].numpy()
    t0 = time.perf_counter()
    host_found = [sorted(detect_markers_numpy(f, dictionary="DICT_ARUCO_ORIGINAL")[1].reshape(-1).tolist())
                  for f in frames_np]
    host_ms = (time.perf_counter() - t0) * 1e3 / n
    pinned = host["typical"][0].pin_memory()
    target = torch.empty_like(dev["typical"][0])
    ups = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        target.copy_(pinned, non_blocking=True)
        torch.cuda.synchronize()
        ups.append((time.perf_counter() - t0) * 1e3)
    upload_ms = statistics.median(ups[1:])

    frame_bytes = B * H * W * 3
    res = {"shape": [B, H, W], "kw": KW, "rotate": a.rotate, "iters": a.iters, "windows": a.windows, "checks": checks,
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()},
           "host_numpy_ms_per_frame": host_ms, "host_numpy_ms_per_batch": host_ms * B,
           "host_found_of_planted": [sum(len(f) for f in host_found), sum(len(p) for p in host["typical"][1][:n])],
           "upload_ms_per_batch": upload_ms}
    med = {k: v["median"] for k, v in res["ms"].items()}
    res["read_tbps"] = {k: frame_bytes / (med[k] * 1e-3) / 1e12 for k in ("range", "mask")}
    res["share_of_read_roof"] = {k: v / READ_ROOF_TBPS for k, v in res["read_tbps"].items()}
    res["copy_tbps"] = 2 * frame_bytes / (med["copy"] * 1e-3) / 1e12
    res["copy_share_of_copy_roof"] = res["copy_tbps"] / COPY_ROOF_TBPS
    res["step_over_copy"] = med["step"] / med["copy"]
    res["host_over_step"] = host_ms * B / med["step"]
    res["host_over_step_with_upload"] = host_ms * B / (med["step"] + upload_ms)
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
