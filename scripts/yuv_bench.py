"""yuv_to_rgb at the YOLO bench shape against a plain copy of the same bytes and against the host
path it replaces (profiles/yuv_to_rgb.md).

B raw frames of H x W random bytes per layout (nv12, i420, i444, yuyv).  Per layout:

* (a) ``yuv_to_rgb`` into a preallocated batch; (b) ``dst.copy_(src)`` of uint8 tensors moving the
  same total bytes (raw in + RGB out: the copy reads half of them and writes half) on the same
  card, the roof of (a): device events around ``--iters`` back-to-back calls (one hipGraph of them,
  so that the host's launch time stays out) after 10 warm-ups, in ``--windows`` windows (median
  and spread reported);
* (c) the host path: the numpy converter of the media elements on each of the B frames
  (``v4l2.yuyv_to_rgb`` for yuyv, the plane handling of ``iter_y4m`` + ``video_io._yuv_to_rgb`` for
  the planar layouts, nv12 de-interleaved first), then ``FrameUpload`` of the RGB batch — against
  (d) ``FrameUpload`` of the raw batch with ``format`` set + ``YuvToRgb``.  Host clock around each,
  device synchronised, one repetition.  Note that (c) rounds as its standard says (bt601 for yuyv,
  jpeg for the planar ones) and (d) is run with the same standard.

Usage:  python scripts/yuv_bench.py [--out FILE.json]
"""
import argparse
import json
import os
import queue
import statistics
import sys
import time

import numpy as np
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


def host_convert(fmt, frame, h, w):
    """One raw frame (1-D uint8 numpy) -> RGB [H, W, 3] as the media elements do it today."""
    from aiko_services_amd.elements.media import v4l2, video_io
    if fmt == "yuyv":
        return v4l2.yuyv_to_rgb(frame, w, h)
    y = frame[:h * w].reshape(h, w)
    if fmt == "i444":
        return video_io._yuv_to_rgb(y, frame[h * w:2 * h * w].reshape(h, w), frame[2 * h * w:].reshape(h, w))
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if fmt == "nv12":
        c = frame[h * w:].reshape(ch, cw, 2)
        u, v = c[..., 0], c[..., 1]
    else:
        u = frame[h * w:h * w + ch * cw].reshape(ch, cw)
        v = frame[h * w + ch * cw:].reshape(ch, cw)
    u = u.repeat(2, 0).repeat(2, 1)[:h, :w]
    v = v.repeat(2, 0).repeat(2, 1)[:h, :w]
    return video_io._yuv_to_rgb(y, u, v)


def elements(fmt, standard, h, w):
    """(FrameUpload rgb, FrameUpload raw, YuvToRgb) elements of two one-off pipelines."""
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    vision, ingest = "aiko_services_amd.elements.gpu.vision", "aiko_services_amd.elements.gpu.ingest"
    io = {"input": [{"name": "images", "type": "tensor"}], "output": [{"name": "images", "type": "tensor"}]}

    def make(name, graph, els):
        d = {"version": 0, "name": name, "runtime": "python", "graph": [graph], "parameters": {}, "elements": els}
        return PipelineImpl.create_pipeline(f"<{name}>", parse_pipeline_definition_dict(d), None, None, "b", [], 0,
                                            None, 60, queue_response=queue.Queue())

    p1 = make(f"p_rgb_{fmt}", "(FrameUpload)", [dict(io, name="FrameUpload", parameters={"pool": 2},
                                                      deploy={"local": {"module": vision}})])
    p2 = make(f"p_raw_{fmt}", "(FrameUpload YuvToRgb)", [
        dict(io, name="FrameUpload", parameters={"pool": 2, "format": fmt, "height": h, "width": w},
             deploy={"local": {"module": vision}}),
        dict(io, name="YuvToRgb", parameters={"format": fmt, "standard": standard, "height": h, "width": w},
             deploy={"local": {"module": ingest}})])
    get = lambda p, n: p.pipeline_graph.get_node(n).element  # noqa: E731
    return get(p1, "FrameUpload"), get(p2, "FrameUpload"), get(p2, "YuvToRgb")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-host", action="store_true", help="leave (c) and (d), the host comparison, out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yuv_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd.ops import require_native
    from aiko_services_amd.ops import yuv as Y
    require_native()
    B, H, W = a.batch, a.height, a.width
    g = torch.Generator().manual_seed(a.seed)
    rows = []
    for fmt in FMTS:
        n = Y.frame_bytes(fmt, H, W)
        raw_h = torch.randint(0, 256, (B, n), dtype=torch.uint8, generator=g)
        raw = raw_h.cuda()
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
        vector = Y.uses_vector(raw, out, W)
        ta = timed(lambda: Y.yuv_to_rgb(raw, H, W, fmt, "bt601", out=out), a.iters, a.windows)
        total = raw.numel() + out.numel()
        src = torch.empty(total // 2, dtype=torch.uint8, device="cuda").random_(0, 256)
        dst = torch.empty_like(src)
        tb = timed(lambda: dst.copy_(src), a.iters, a.windows)
        del src, dst
        row = {"format": fmt, "vector": vector, "bytes_in": raw.numel(), "bytes_out": out.numel(),
               "a_yuv_to_rgb": ta, "b_copy_same_bytes": tb, "a_over_b": round(ta["median_us"] / tb["median_us"], 3),
               "GBps_a": round(total / ta["median_us"] / 1e3, 1), "GBps_b": round(total / tb["median_us"] / 1e3, 1)}
        if not a.skip_host:
            standard = "bt601" if fmt == "yuyv" else "jpeg"
            up_rgb, up_raw, conv = elements(fmt, standard, H, W)
            frames = [f for f in raw_h.numpy()]
            # warm both paths up on the whole batch shape (pools, staging sets, first launch)
            warm = np.zeros((B, H, W, 3), np.uint8)
            up_rgb.process_frame(None, images=warm)
            conv.process_frame(None, images=up_raw.process_frame(None, images=frames)[1]["images"])
            host_convert(fmt, frames[0], H, W)
            torch.cuda.synchronize()
            t = time.perf_counter()
            rgb = [host_convert(fmt, f, H, W) for f in frames]
            t_conv = time.perf_counter() - t
            _, o = up_rgb.process_frame(None, images=rgb)
            torch.cuda.synchronize()
            tc = time.perf_counter() - t
            host_result = o["images"].clone()
            t = time.perf_counter()
            _, o = up_raw.process_frame(None, images=frames)
            _, o = conv.process_frame(None, images=o["images"])
            torch.cuda.synchronize()
            td = time.perf_counter() - t
            row.update(c_host_convert_upload_us=round(tc * 1e6, 1), c_convert_only_us=round(t_conv * 1e6, 1),
                       d_raw_upload_kernel_us=round(td * 1e6, 1), c_over_d=round(tc / td, 1),
                       uploaded_rgb=up_rgb.bytes_uploaded // 2, uploaded_raw=up_raw.bytes_uploaded // 2,
                       device_equals_host=bool(torch.equal(o["images"], host_result)))
        rows.append(row)
    res = {"shape": {"B": B, "H": H, "W": W}, "iters": a.iters, "windows": a.windows,
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
