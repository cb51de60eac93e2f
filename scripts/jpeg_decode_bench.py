"""jpeg_decode at the YOLO bench shape: the decode of three kinds of stream, its three passes alone, a
plain copy of the raw frames it writes, and the host path it replaces (profiles/jpeg_decode.md).

B frames of H x W, 4:2:0, quality 90, frames with structure (``jpeg_bench.structured_frames``).  In one run:

* the decode (``ops.jpeg_decode.jpeg_decode`` with every output and the workspace preallocated) of (a) this
  project's encoder's streams (one restart interval per MCU row, one descriptor for all frames), (b)
  Pillow streams with ``restart_marker_rows=1`` and (c) Pillow streams without ``DRI`` (one lane per frame);
* (d) the three passes alone on (a) (``aiko_jpeg_decode_pass`` of the built library, called directly);
* (e) ``out.copy_(raw)`` of the raw frames;
* all of them timed by device events around ``--iters`` back-to-back calls after a warm-up of 10, in
  ``--windows`` windows; the windows of the variants alternate; median and spread reported;
* once, by the host clock: (f) the path replaced, Pillow's decode of every frame of (b) and the upload of
  the RGB frames, against (g) ``pack`` of (b) into pinned memory, the upload of the coded bytes and the
  decode; the host cost of ``pack`` alone;
* ``torch.equal`` of the benched output with ``jpeg_decode_ref`` on one frame of each kind, and the
  statuses.

Usage:  python scripts/jpeg_decode_bench.py [--out FILE.json]
"""
import argparse
import ctypes
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from jpeg_bench import structured_frames, timed_together  # noqa: E402


def decode_pass():
    """``fn(index, ...)`` launching one pass of jpeg_decode_ops.hip on the current stream."""
    import aiko_services_amd
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(aiko_services_amd.__file__)), "_C.so"))
    one = lib.aiko_jpeg_decode_pass
    one.restype = ctypes.c_int
    one.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 3 + \
        [ctypes.c_int] * 4 + [ctypes.c_long, ctypes.c_int, ctypes.c_void_p]

    def fn(index, data, nbytes, desc, workspace, raw, status, H, W, max_intervals):
        rc = one(index, data.data_ptr(), nbytes.data_ptr(), desc.data_ptr(), desc.shape[0], workspace.data_ptr(),
                 raw.data_ptr(), status.data_ptr(), data.shape[0], H, W, 1, data.shape[1], max_intervals,
                 torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"aiko_jpeg_decode_pass({index}) returned {rc}")

    fn.keep = lib
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench: needs a GPU (nothing is measured on the CPU)")
    from PIL import Image

    from aiko_services_amd.ops import jpeg as J
    from aiko_services_amd.ops import jpeg_decode as D
    from aiko_services_amd.ops import require_native
    from aiko_services_amd.ops.reference import jpeg_decode_ref
    from aiko_services_amd.ops.yuv import frame_bytes, rgb_to_yuv
    require_native()
    one_pass = decode_pass()
    B, H, W, fmt, quality = a.batch, a.height, a.width, "i420", a.quality
    dev = "cuda"
    rgb = structured_frames(B, H, W, a.seed + 1, dev)
    host_rgb = rgb.cpu().numpy()

    def pillow(**kw):
        out = []
        for f in host_rgb:
            buf = io.BytesIO()
            Image.fromarray(f, "RGB").save(buf, format="JPEG", quality=quality, subsampling=2, **kw)
            out.append(buf.getvalue())
        return out

    coded = {"b_pillow_rst_rows": pillow(restart_marker_rows=1), "c_pillow_no_dri": pillow()}
    sets, plans = {}, {}
    stream, lengths = J.jpeg_encode(rgb_to_yuv(rgb, fmt, "jpeg"), H, W, fmt, quality)
    plans["a_ours"] = D.parse(J.header(fmt, H, W, quality))
    sets["a_ours"] = (stream, lengths, D.plan_bytes(plans["a_ours"])[None].to(dev))
    for kind, frames in coded.items():
        data, nbytes, desc, plans[kind] = D.pack(frames)
        sets[kind] = (data.to(dev), nbytes.to(dev), desc.to(dev))
    raw = {k: torch.empty(B, frame_bytes(fmt, H, W), dtype=torch.uint8, device=dev) for k in sets}
    status = {k: torch.empty(B, dtype=torch.int32, device=dev) for k in sets}
    works = {k: torch.empty(D.workspace_bytes(fmt, H, W, B, plans[k].restart_interval), dtype=torch.uint8, device=dev)
             for k in sets}

    def decode(kind):
        return D.jpeg_decode(*sets[kind], H, W, fmt, restart_interval=plans[kind].restart_interval, raw=raw[kind],
                             status=status[kind], workspace=works[kind])

    nint = D.intervals(fmt, H, W, plans["a_ours"].restart_interval)
    side_raw, side_status = torch.empty_like(raw["a_ours"]), torch.empty_like(status["a_ours"])
    copy_out = torch.empty_like(raw["a_ours"])
    fns = {kind: (lambda kind=kind: decode(kind)) for kind in sets}
    for index, name in enumerate(("d_scan_pass", "d_entropy_pass", "d_idct_pass")):
        fns[name] = lambda index=index: one_pass(index, *sets["a_ours"], works["a_ours"], side_raw, side_status, H, W, nint)
    fns["e_copy_raw"] = lambda: copy_out.copy_(raw["a_ours"])
    decode("a_ours")                                        # the passes alone read its workspace
    t = timed_together(fns, a.iters, a.windows)

    checks, sizes = {}, {}
    for kind, (data, nbytes, desc) in sets.items():
        decode(kind)
        torch.cuda.synchronize()
        n = nbytes.cpu()
        sizes[kind] = {"mean_bytes": round(float(n.float().mean()), 1), "max_bytes": int(n.max()),
                       "intervals": D.intervals(fmt, H, W, plans[kind].restart_interval)}
        checks[f"{kind}_status_all_zero"] = not bool(status[kind].any())
        want = jpeg_decode_ref(data[:1].cpu(), n[:1], desc[:1].cpu(), H, W, fmt)
        checks[f"{kind}_frame_equals_reference"] = bool(torch.equal(raw[kind][:1].cpu(), want[0])) and not bool(want[1].any())
    checks["passes_equal_operator"] = bool(torch.equal(side_raw, raw["a_ours"])) and bool(torch.equal(side_status, status["a_ours"]))

    # the host clock: the path replaced against the new one, on the Pillow streams with restart intervals
    frames = coded["b_pillow_rst_rows"]
    pinned_rgb = torch.empty(B, H, W, 3, dtype=torch.uint8, pin_memory=True)
    dev_rgb = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    Image.open(io.BytesIO(frames[0])).convert("RGB")        # warms Pillow up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = pinned_rgb.numpy()
    for k, f in enumerate(frames):
        rows[k] = Image.open(io.BytesIO(f)).convert("RGB")
    t_decode = time.perf_counter()
    dev_rgb.copy_(pinned_rgb, non_blocking=True)
    torch.cuda.synchronize()
    f_host_us, f_decode_us = (time.perf_counter() - t0) * 1e6, (t_decode - t0) * 1e6
    cap = sets["b_pillow_rst_rows"][0].shape[1]
    pinned = (torch.zeros(B, cap, dtype=torch.uint8, pin_memory=True), torch.zeros(B, dtype=torch.int32, pin_memory=True),
              torch.zeros(B, D.PLAN_BYTES, dtype=torch.uint8, pin_memory=True))
    D.pack(frames, out=pinned)                              # warms the header cache up, as a stream's second batch is
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    D.pack(frames, out=pinned)
    t_pack = time.perf_counter()
    for dst, src in zip(sets["b_pillow_rst_rows"], pinned):
        dst.copy_(src, non_blocking=True)
    decode("b_pillow_rst_rows")
    torch.cuda.synchronize()
    g_new_us, g_pack_us = (time.perf_counter() - t0) * 1e6, (t_pack - t0) * 1e6

    med = {k: v["median_us"] for k, v in t.items()}
    res = {"shape": {"B": B, "H": H, "W": W, "format": fmt, "quality": quality}, "iters": a.iters, "windows": a.windows,
           "raw_bytes": raw["a_ours"].numel(), "rgb_bytes": dev_rgb.numel(),
           "workspace_bytes": {k: w.numel() for k, w in works.items()}, "us": t, "streams": sizes,
           "a_over_e": round(med["a_ours"] / med["e_copy_raw"], 1), "b_over_e": round(med["b_pillow_rst_rows"] / med["e_copy_raw"], 1),
           "c_over_a": round(med["c_pillow_no_dri"] / med["a_ours"], 1),
           "a_frames_per_second": round(B / med["a_ours"] * 1e6),
           "f_host_path_us": round(f_host_us, 1), "f_pillow_decode_us": round(f_decode_us, 1),
           "g_new_path_us": round(g_new_us, 1), "g_pack_us": round(g_pack_us, 1),
           "g_coded_bytes": int(sets["b_pillow_rst_rows"][1].sum()),
           "f_over_g": round(f_host_us / g_new_us, 1),
           "f_decode_over_a": round(f_decode_us / med["a_ours"], 1), "f_decode_over_b": round(f_decode_us / med["b_pillow_rst_rows"], 1),
           "f_decode_over_c": round(f_decode_us / med["c_pillow_no_dri"], 2),
           "checks": checks}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
