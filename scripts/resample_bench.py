"""resample at the Whisper bench shape against a plain copy of the same bytes and against the host
path it replaces (profiles/audio_resample.md).  The method of scripts/yuv_bench.py.

B streams of ``--seconds`` of random stereo int16 PCM.  Per input rate (48 kHz, 44.1 kHz -> 16 kHz):

* (a) ``ops.audio.resample`` into preallocated outputs on the vector kernel; (b) ``dst.copy_(src)``
  of uint8 tensors moving the same total bytes (pcm and hist in, out and hist_out out) on the same
  card; (e) ``resample`` of a pcm view one int16 off alignment, which the scalar kernel serves:
  device events around ``--iters`` back-to-back calls (one hipGraph of them, so that the host's
  launch time stays out) after 10 warm-ups, in ``--windows`` windows (median and spread reported);
* (c) the host path: per stream ``read_wav``'s normalisation and channel mean, then
  ``resample_linear``, then the fp32 upload — against (d) the int16 upload, then the kernel.  Host
  clock around each, device synchronised, one repetition after one warm-up.
* ``--variant-lib NAME=FILE``: a shared object built from ``csrc/kernels/resample_ops.hip`` alone with
  other ``-D`` options (``-DAIKO_RS_CHAINS=8``: eight outputs per thread), exporting
  ``aiko_resample``; timed like (a) next to it, its output compared with (a)'s.  Several allowed.

* ``--pipeline``: instead of the above, the Whisper-small bench pipeline (``bench.whisper_definition``:
  28 streams, 5 s chunks, 30 s windows) as it is, fed fp32 16 kHz chunks, against the same pipeline
  fed 48 kHz stereo int16 chunks through ``AudioResample``; both pools are synthetic and in HBM.
  ``--steps`` timed frames after 8 set-up and 10 warm-up frames, two frames in flight, the two
  pipelines alternating ``--windows`` times in one process; host clock, device synchronised.

Usage:  python scripts/resample_bench.py [--pipeline] [--out FILE.json]
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


def host_convert(pcm, rate_in, rate_out):
    """int16 [B, n, C] (numpy) -> fp32 [B, n_out]: what ``AudioReadFile`` does per file on the host."""
    from aiko_services_amd.elements.media.audio_io import resample_linear
    rows = []
    for x in pcm:
        m = (x.astype(np.float32) / np.float32(32768.0)).mean(axis=1)
        rows.append(resample_linear(m, rate_in, rate_out))
    return np.stack(rows)


def variant(path):
    """``fn(pcm, hist, filt, L, M, out, hist_out)`` launching ``aiko_resample`` of the shared object."""
    lib = ctypes.CDLL(os.path.abspath(path))
    entry = lib.aiko_resample
    entry.restype = ctypes.c_int
    entry.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_long] + \
        [ctypes.c_int] * 4 + [ctypes.c_void_p]

    def fn(pcm, hist, filt, L, M, out, hist_out):
        B, n_in, C = pcm.shape
        rc = entry(pcm.data_ptr(), int(pcm.dtype == torch.float32), hist.data_ptr(), filt.data_ptr(), out.data_ptr(),
                   hist_out.data_ptr(), B, n_in, C, L, M, filt.shape[1], torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"{path}: aiko_resample returned {rc}")

    fn.keep = lib
    return fn


def pipeline_times(a):
    import queue
    from collections import deque

    import bench
    from aiko_services_amd.pipeline.definition import parse_pipeline_definition_dict
    from aiko_services_amd.pipeline.engine import PipelineImpl
    plain = bench.whisper_definition(a.streams, True, "small", a.seconds, 30.0)
    raw = bench.whisper_definition(a.streams, True, "small", a.seconds, 30.0)
    raw["name"] = "p_whisper_encoder_pcm16"
    raw["graph"] = ["(AudioChunks AudioResample AudioWindow WhisperEncoder FeatureSink)"]
    raw["elements"][0]["parameters"].update(format="pcm16", sample_rate=a.rates[0], channels=a.channels)
    raw["elements"].insert(1, {
        "name": "AudioResample", "input": [{"name": "audio", "type": "tensor"}],
        "output": [{"name": "audio", "type": "tensor"}],
        "parameters": {"sample_rate_in": a.rates[0], "sample_rate_out": a.rate_out, "channels": a.channels},
        "deploy": {"local": {"module": "aiko_services_amd.elements.gpu.audio_ingest"}}})
    runs = {}
    for name, d in (("f32_16k", plain), ("pcm16_resample", raw)):
        q = queue.Queue()
        p = PipelineImpl.create_pipeline("<bench>", parse_pipeline_definition_dict(d), None, None, name, [], 0, None,
                                         3600, queue_response=q)
        runs[name] = {"pipeline": p, "queue": q, "frame": 0, "ms_per_step": []}

    def steps(r, name, n):
        inflight = deque()
        for _ in range(n):
            r["pipeline"].process_frame({"stream_id": name, "frame_id": r["frame"]}, {})
            r["frame"] += 1
            info, out = r["queue"].get_nowait()
            if info["state"] != 0:
                raise RuntimeError(f"pipeline frame failed: {info} {out}")
            inflight.append(out["embedding"])
            while len(inflight) > 2:
                inflight.popleft().wait()
        while inflight:
            inflight.popleft().wait()
        torch.cuda.synchronize()

    for name, r in runs.items():
        steps(r, name, 8)
        steps(r, name, 10)
    for _ in range(a.windows):
        for name, r in runs.items():
            t = time.perf_counter()
            steps(r, name, a.steps)
            r["ms_per_step"].append(round((time.perf_counter() - t) * 1e3 / a.steps, 3))
    res = {"pipeline": True, "streams": a.streams, "chunk_s": a.seconds, "rate_in": a.rates[0], "channels": a.channels,
           "steps": a.steps}
    for name, r in runs.items():
        res[name] = {"ms_per_step": r["ms_per_step"], "median_ms": statistics.median(r["ms_per_step"]),
                     "windows_per_s": round(a.streams / statistics.median(r["ms_per_step"]) * 1e3, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=28)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--rates", type=int, nargs="+", default=[48000, 44100])
    ap.add_argument("--rate-out", type=int, default=16000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-host", action="store_true", help="leave (c) and (d), the host comparison, out")
    ap.add_argument("--variant-lib", action="append", default=[], help="name=FILE.so, see above")
    ap.add_argument("--pipeline", action="store_true", help="time the Whisper-small pipeline with and without it")
    ap.add_argument("--steps", type=int, default=40, help="timed frames per window of --pipeline")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd.ops import audio as A
    from aiko_services_amd.ops import require_native
    require_native()
    if a.pipeline:
        line = json.dumps(pipeline_times(a))
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    B, C = a.streams, a.channels
    rows = []
    for rate in a.rates:
        filt_h, L, M = A.resample_filter(rate, a.rate_out)
        T = filt_h.shape[1]
        n_in = int(a.seconds * rate)
        n_out = n_in * L // M
        g = torch.Generator().manual_seed(a.seed + rate)
        pcm_h = torch.randint(-32768, 32768, (B, n_in, C), generator=g).to(torch.int16)
        pcm, filt = pcm_h.cuda(), filt_h.cuda()
        hist = torch.rand(B, T - 1, generator=g).cuda()
        out = torch.empty(B, n_out, device="cuda")
        hist_out = torch.empty(B, T - 1, device="cuda")
        vector = A.resample_uses_vector(pcm)
        ta = timed(lambda: A.resample(pcm, hist, filt, L, M, out=out, hist_out=hist_out), a.iters, a.windows)
        result = (out.clone(), hist_out.clone())
        total = pcm.numel() * 2 + 4 * (hist.numel() + out.numel() + hist_out.numel())
        src = torch.empty(total // 2, dtype=torch.uint8, device="cuda").random_(0, 256)
        dst = torch.empty_like(src)
        tb = timed(lambda: dst.copy_(src), a.iters, a.windows)
        del src, dst
        off = torch.empty(pcm.numel() + 8, dtype=torch.int16, device="cuda")[1:1 + pcm.numel()].view(pcm.shape)
        off.copy_(pcm)
        assert not A.resample_uses_vector(off)
        out_e = torch.empty_like(out)
        te = timed(lambda: A.resample(off, hist, filt, L, M, out=out_e, hist_out=hist_out), a.iters, a.windows)
        macs = B * n_out * T
        row = {"rate_in": rate, "L": L, "M": M, "T": T, "n_in": n_in, "n_out": n_out, "vector": vector,
               "lds_bytes": A.resample_lds_bytes(L, M, T), "grid": list(A.resample_grid(n_out, B)),
               "bytes_moved": total, "a_resample": ta, "b_copy_same_bytes": tb,
               "a_over_b": round(ta["median_us"] / tb["median_us"], 3),
               "GBps_a": round(total / ta["median_us"] / 1e3, 1), "GBps_b": round(total / tb["median_us"] / 1e3, 1),
               "GFLOPs_a": round(2 * macs / ta["median_us"] / 1e3, 1),
               "e_scalar_kernel": te, "scalar_equals_vector": bool(torch.equal(out_e, result[0]))}
        del off, out_e
        for spec in a.variant_lib:
            name, _, path = spec.partition("=")
            fn = variant(path)
            other, other_h = torch.zeros_like(out), torch.zeros_like(hist_out)
            row[f"variant_{name}"] = timed(lambda: fn(pcm, hist, filt, L, M, other, other_h), a.iters, a.windows)
            row[f"variant_{name}_equal"] = bool(torch.equal(other, result[0]) and torch.equal(other_h, result[1]))
        if not a.skip_host:
            pcm_n = pcm_h.numpy()
            host_convert(pcm_n[:1], rate, a.rate_out)
            torch.cuda.synchronize()
            t = time.perf_counter()
            mono = host_convert(pcm_n, rate, a.rate_out)
            t_conv = time.perf_counter() - t
            up = torch.from_numpy(mono).cuda()
            torch.cuda.synchronize()
            tc = time.perf_counter() - t
            t = time.perf_counter()
            A.resample(pcm_h.cuda(), hist, filt, L, M, out=out, hist_out=hist_out)
            torch.cuda.synchronize()
            td = time.perf_counter() - t
            row.update(c_host_convert_upload_us=round(tc * 1e6, 1), c_host_convert_only_us=round(t_conv * 1e6, 1),
                       d_int16_upload_kernel_us=round(td * 1e6, 1), c_over_d=round(tc / td, 1),
                       host_shape_equals_device=bool(tuple(up.shape) == tuple(out.shape)))
        rows.append(row)
    res = {"shape": {"streams": B, "seconds": a.seconds, "channels": C, "rate_out": a.rate_out}, "iters": a.iters,
           "windows": a.windows,
           "tile": {"threads": A.RESAMPLE_THREADS, "chains": A.RESAMPLE_CHAINS, "tile": A.RESAMPLE_TILE},
           "rates": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
