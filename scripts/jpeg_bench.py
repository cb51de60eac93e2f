"""jpeg_encode at the YOLO bench shape: the encode against a plain copy of the same raw bytes, the
rgb_to_yuv launch in front of it, and the host path it replaces (profiles/jpeg_encode.md).

B frames of H x W, ``i420``, quality 90, the default capacities.  In one run:

* the encode (``ops.jpeg.jpeg_encode`` with every output and the workspace preallocated) on (a) noise
  (uint8 RGB noise through ``rgb_to_yuv``) and (b) frames with structure (per frame a different mix of
  gradients, waves, flat rectangles with hard edges and a little noise);
* its two passes alone on (b) (``aiko_jpeg_rows`` / ``aiko_jpeg_assemble`` of the built library,
  called directly);
* (c) ``out.copy_(raw)`` of the same raw bytes and (d) the ``rgb_to_yuv`` launch that produces them;
* all of them timed by device events around ``--iters`` back-to-back calls after a warm-up of 10, in
  ``--windows`` windows; the windows of the variants alternate; median and spread reported;
* (e) once, by the host clock: the RGB frames to the host and ``AviWriter._encode`` (Pillow) of
  every frame at the same quality;
* bytes out per frame, and ``torch.equal`` of the benched output with ``jpeg_encode_ref`` on two
  frames of each kind.

Usage:  python scripts/jpeg_bench.py [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def passes():
    """``(rows_fn, assemble_fn)`` launching the two passes of jpeg_ops.hip on the current stream."""
    import aiko_services_amd
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(aiko_services_amd.__file__)), "_C.so"))
    rows, assemble = lib.aiko_jpeg_rows, lib.aiko_jpeg_assemble
    rows.restype = assemble.restype = ctypes.c_int
    rows.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    assemble.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] + \
        [ctypes.c_int] * 4 + [ctypes.c_long, ctypes.c_int, ctypes.c_void_p]

    def rows_fn(raw, tables, workspace, H, W, seg_cap):
        rc = rows(raw.data_ptr(), tables.data_ptr(), workspace.data_ptr(), raw.shape[0], H, W, 1, seg_cap,
                  torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"aiko_jpeg_rows returned {rc}")

    def assemble_fn(tables, head, workspace, stream, nbytes, H, W, seg_cap):
        rc = assemble(tables.data_ptr(), head, workspace.data_ptr(), stream.data_ptr(), nbytes.data_ptr(),
                      stream.shape[0], H, W, 1, stream.shape[1], seg_cap, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"aiko_jpeg_assemble returned {rc}")

    rows_fn.keep = lib
    return rows_fn, assemble_fn


def structured_frames(B, H, W, seed, device):
    """uint8 ``[B, H, W, 3]``: per frame other gradients and waves, six flat rectangles, noise of sigma 3."""
    g = torch.Generator(device=device).manual_seed(seed)
    yy = torch.arange(H, device=device, dtype=torch.float32).view(1, H, 1)
    xx = torch.arange(W, device=device, dtype=torch.float32).view(1, 1, W)
    k = torch.rand(B, 6, generator=g, device=device).view(B, 6, 1, 1)
    r = 128 + 90 * torch.sin(xx / (20 + 60 * k[:, 0]) + yy / (40 + 80 * k[:, 1]))
    gch = 128 + 90 * torch.cos(yy / (15 + 50 * k[:, 2]) + 3 * k[:, 3]) + 0 * xx
    bch = 40 + 170 * (xx * k[:, 4] / W + yy * (1 - k[:, 4]) / H) + 0 * k[:, 5]
    out = torch.stack([r, gch, bch], -1)
    boxes = torch.randint(0, 10 ** 6, (B, 6, 5), generator=g, device=device).cpu()
    for b in range(B):
        for y, x, h, w, c in boxes[b].tolist():
            y, x, h, w = y % (H - 40), x % (W - 60), 16 + h % 80, 16 + w % 120
            out[b, y:y + h, x:x + w] = float(c % 256)
    out += 3 * torch.randn(out.shape, generator=g, device=device)
    return out.clamp_(0, 255).to(torch.uint8)


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
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-host", action="store_true", help="leave (e), the host path, out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd.elements.media.avi import AviWriter
    from aiko_services_amd.ops import jpeg as J
    from aiko_services_amd.ops import require_native
    from aiko_services_amd.ops.reference import jpeg_encode_ref
    from aiko_services_amd.ops.yuv import rgb_to_yuv
    require_native()
    rows_fn, assemble_fn = passes()
    B, H, W, fmt, quality = a.batch, a.height, a.width, "i420", a.quality
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(a.seed)
    rgb = {"noise": torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=g),
           "structured": structured_frames(B, H, W, a.seed + 1, dev)}
    raw = {k: rgb_to_yuv(v, fmt, "jpeg") for k, v in rgb.items()}
    cap, seg_cap = J.capacities(fmt, H, W)
    stream = {k: torch.empty(B, cap, dtype=torch.uint8, device=dev) for k in raw}
    nbytes = {k: torch.empty(B, dtype=torch.int32, device=dev) for k in raw}
    workspace = torch.empty(J.workspace_bytes(fmt, H, W, B), dtype=torch.uint8, device=dev)
    tables, head = J.device_tables(fmt, H, W, quality, dev)

    def encode(kind):
        return J.jpeg_encode(raw[kind], H, W, fmt, quality, stream=stream[kind], nbytes=nbytes[kind],
                             workspace=workspace)

    copy_out, yuv_out = torch.empty_like(raw["structured"]), torch.empty_like(raw["structured"])
    scratch_stream, scratch_n = torch.empty_like(stream["structured"]), torch.empty_like(nbytes["structured"])
    fns = {"a_encode_noise": lambda: encode("noise"), "b_encode_structured": lambda: encode("structured"),
           "b_rows_pass": lambda: rows_fn(raw["structured"], tables, workspace, H, W, seg_cap),
           "c_copy_raw": lambda: copy_out.copy_(raw["structured"]),
           "d_rgb_to_yuv": lambda: rgb_to_yuv(rgb["structured"], fmt, "jpeg", out=yuv_out)}
    t = timed_together(fns, a.iters, a.windows)
    # the assembly needs the structured frames' segments in the workspace: timed after them, alone
    encode("structured")
    t.update(timed_together({"b_assemble_pass": lambda: assemble_fn(tables, head, workspace, scratch_stream, scratch_n,
                                                                     H, W, seg_cap)}, a.iters, a.windows))
    checks, sizes = {}, {}
    for kind in raw:
        encode(kind)
        torch.cuda.synchronize()
        n = nbytes[kind].cpu()
        fit = n[n > 0]
        sizes[kind] = {"overflowed": int((n < 0).sum()), "mean_bytes": round(float(fit.float().mean()), 1) if len(fit) else None,
                       "min_bytes": int(fit.min()) if len(fit) else None, "max_bytes": int(fit.max()) if len(fit) else None}
        want = jpeg_encode_ref(raw[kind][:2].cpu(), H, W, fmt, quality)
        checks[f"{kind}_two_frames_equal_reference"] = bool(torch.equal(n[:2], want[1])) and all(
            bool(torch.equal(stream[kind][b, :int(want[1][b])].cpu(), want[0][b, :int(want[1][b])]))
            for b in range(2) if int(want[1][b]) > 0)
    checks["passes_equal_operator"] = bool(torch.equal(scratch_n, nbytes["structured"])) and all(
        bool(torch.equal(scratch_stream[b, :int(scratch_n[b])], stream["structured"][b, :int(scratch_n[b])]))
        for b in range(0, B, max(1, B // 8)))

    host_us = host_bytes = None
    if not a.skip_host:
        with tempfile.TemporaryDirectory() as tmp:
            writer = AviWriter(os.path.join(tmp, "x.avi"), W, H, 30.0, "MJPG", quality)
            writer._encode(rgb["structured"][0].cpu().numpy())              # warms Pillow up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frames = rgb["structured"].cpu().numpy()                        # the sync
            host_bytes = sum(len(writer._encode(f)[1]) for f in frames)
            host_us = (time.perf_counter() - t0) * 1e6
            writer.close()

    raw_bytes = raw["structured"].numel()
    res = {"shape": {"B": B, "H": H, "W": W, "format": fmt, "quality": quality, "cap": cap, "seg_cap": seg_cap},
           "iters": a.iters, "windows": a.windows, "raw_bytes": raw_bytes, "workspace_bytes": workspace.numel(),
           "us": t, "bytes_per_frame": sizes,
           "a_over_c": round(t["a_encode_noise"]["median_us"] / t["c_copy_raw"]["median_us"], 2),
           "b_over_c": round(t["b_encode_structured"]["median_us"] / t["c_copy_raw"]["median_us"], 2),
           "b_raw_read_GBps": round(raw_bytes / t["b_encode_structured"]["median_us"] / 1e3, 1),
           "b_frames_per_second": round(B / t["b_encode_structured"]["median_us"] * 1e6),
           "e_host_us": None if host_us is None else round(host_us, 1),
           "e_host_bytes_per_frame": None if host_bytes is None else round(host_bytes / B, 1),
           "e_over_b": None if host_us is None else round(host_us / t["b_encode_structured"]["median_us"], 1),
           "checks": checks}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
