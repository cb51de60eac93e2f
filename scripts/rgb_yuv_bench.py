"""rgb_to_yuv at the YOLO bench shape against a plain copy of the same bytes and against the host
path it replaces (profiles/rgb_to_yuv.md).  The method of scripts/yuv_bench.py.

B RGB frames of H x W random pixels.  Per layout (nv12, i420, i444, yuyv):

* (a) ``rgb_to_yuv`` into a preallocated batch on the vector kernel; (b) ``dst.copy_(src)`` of uint8
  tensors moving the same total bytes (RGB in + raw out) on the same card; (e) ``rgb_to_yuv`` into
  an output one byte off alignment, which the byte kernel serves: device events around ``--iters``
  back-to-back calls (one hipGraph of them, so that the host's launch time stays out) after 10
  warm-ups, in ``--windows`` windows (median and spread reported);
* (c) the host path: download of the RGB batch, then ``video_io._rgb_to_yuv`` (and, for the
  subsampled layouts, the block means of ``video_io._rgb_to_yuv420``) on each of the B frames —
  against (d) the kernel, then the download of the raw batch.  Host clock around each, device
  synchronised, one repetition.
* ``--variant-lib FILE``: a shared object built from ``csrc/kernels/yuv_out_ops.hip`` alone with
  other ``-D`` options (``-DAIKO_RGB_YUV_LDS_LOAD=0``: every lane loads its own 48 bytes), exporting
  ``aiko_rgb_to_yuv_u8``; timed like (a) next to it, its output compared with (a)'s.  Several allowed.

Usage:  python scripts/rgb_yuv_bench.py [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FMTS = ["nv12", "i420", "i444", "yuyv"]


def timed(fn, iters, windows):
    """Microseconds per call: device events around ``iters`` back-to-back calls, per window.  The
    calls are captured into one hipGraph and replayed: a call takes about as long as its launch
    through Python does, and the graph keeps the host out of the window."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(10):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    runs = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        graph.replay()
        t1.record()
        torch.cuda.synchronize()
        runs.append(t0.elapsed_time(t1) * 1e3 / iters)
    return {"median_us": round(statistics.median(runs), 2), "min_us": round(min(runs), 2),
            "max_us": round(max(runs), 2)}


def host_convert(fmt, frame):
    """One RGB frame [H, W, 3] (numpy) -> packed raw bytes, on the host."""
    import numpy as np

    from aiko_services_amd.elements.media import video_io
    if fmt == "i444":
        return np.concatenate([p.ravel() for p in video_io._rgb_to_yuv(frame)])
    if fmt == "yuyv":
        y = video_io._rgb_to_yuv(frame)[0]
        mean = (frame[:, 0::2].astype(np.int32) + frame[:, 1::2]).astype(np.float32) * np.float32(0.5)
        _, u, v = video_io._rgb_to_yuv(mean)
        return np.stack([y[:, 0::2], u, y[:, 1::2], v], -1).ravel()
    y, u, v = video_io._rgb_to_yuv420(frame)
    if fmt == "nv12":
        return np.concatenate([y.ravel(), np.stack([u, v], -1).ravel()])
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()])


def variant(path, Y, fmt, standard):
    """``fn(rgb, out)`` launching ``aiko_rgb_to_yuv_u8`` of the shared object at ``path``."""
    lib = ctypes.CDLL(os.path.abspath(path))
    entry = lib.aiko_rgb_to_yuv_u8
    entry.restype = ctypes.c_int
    entry.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int,
                                                                             ctypes.c_void_p]
    coeffs, rounding = Y.ENCODE_STANDARDS[standard]
    coef = (ctypes.c_float * 10)(*coeffs)

    def fn(rgb, out):
        B, H, W, _ = rgb.shape
        rc = entry(rgb.data_ptr(), out.data_ptr(), B, H, W, Y.FORMATS[fmt], ctypes.addressof(coef),
                   Y.ROUND_MODES[rounding], torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"{path}: aiko_rgb_to_yuv_u8 returned {rc}")

    fn.keep = (lib, coef)
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--standard", default="bt601")
    ap.add_argument("--skip-host", action="store_true", help="leave (c) and (d), the host comparison, out")
    ap.add_argument("--variant-lib", action="append", default=[], help="name=FILE.so, see above")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rgb_yuv_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd.ops import require_native
    from aiko_services_amd.ops import yuv as Y
    require_native()
    B, H, W = a.batch, a.height, a.width
    g = torch.Generator().manual_seed(a.seed)
    rgb_h = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    rgb = rgb_h.cuda()
    rows = []
    for fmt in FMTS:
        n = Y.frame_bytes(fmt, H, W)
        out = torch.empty(B, n, dtype=torch.uint8, device="cuda")
        vector = Y.encode_uses_vector(rgb, out)
        ta = timed(lambda: Y.rgb_to_yuv(rgb, fmt, a.standard, out=out), a.iters, a.windows)
        result = out.clone()
        total = rgb.numel() + out.numel()
        src = torch.empty(total // 2, dtype=torch.uint8, device="cuda").random_(0, 256)
        dst = torch.empty_like(src)
        tb = timed(lambda: dst.copy_(src), a.iters, a.windows)
        del src, dst
        off = torch.empty(B * n + 16, dtype=torch.uint8, device="cuda")[1:1 + B * n].view(B, n)
        assert not Y.encode_uses_vector(rgb, off)
        te = timed(lambda: Y.rgb_to_yuv(rgb, fmt, a.standard, out=off), a.iters, a.windows)
        row = {"format": fmt, "vector": vector, "bytes_in": rgb.numel(), "bytes_out": out.numel(),
               "a_rgb_to_yuv": ta, "b_copy_same_bytes": tb, "a_over_b": round(ta["median_us"] / tb["median_us"], 3),
               "GBps_a": round(total / ta["median_us"] / 1e3, 1), "GBps_b": round(total / tb["median_us"] / 1e3, 1),
               "e_byte_kernel": te, "byte_equals_vector": bool(torch.equal(off, result))}
        del off
        for spec in a.variant_lib:
            name, _, path = spec.partition("=")
            fn = variant(path, Y, fmt, a.standard)
            other = torch.zeros_like(out)
            row[f"variant_{name}"] = timed(lambda: fn(rgb, other), a.iters, a.windows)
            row[f"variant_{name}_equal"] = bool(torch.equal(other, result))
        if not a.skip_host:
            standard = "jpeg"                                # what the host converter computes
            host_convert(fmt, rgb_h[0].numpy())
            Y.rgb_to_yuv(rgb, fmt, standard, out=out)
            torch.cuda.synchronize()
            t = time.perf_counter()
            frames = rgb.cpu().numpy()
            t_down = time.perf_counter() - t
            raw = [host_convert(fmt, f) for f in frames]
            tc = time.perf_counter() - t
            t = time.perf_counter()
            got = Y.rgb_to_yuv(rgb, fmt, standard, out=out).cpu()
            td = time.perf_counter() - t
            import numpy as np
            row.update(c_download_host_convert_us=round(tc * 1e6, 1), c_download_only_us=round(t_down * 1e6, 1),
                       d_kernel_raw_download_us=round(td * 1e6, 1), c_over_d=round(tc / td, 1),
                       device_equals_host=bool(np.array_equal(got.numpy(), np.stack(raw))))
        rows.append(row)
    res = {"shape": {"B": B, "H": H, "W": W}, "iters": a.iters, "windows": a.windows, "standard": a.standard,
           "tile": {"threads": Y.THREADS, "vector_pixels": Y.VECTOR_PIXELS, "byte_pixels": Y.BYTE_PIXELS},
           "formats": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
