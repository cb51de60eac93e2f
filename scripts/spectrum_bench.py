"""spectrum at the Whisper bench shape against a plain copy of the same bytes, its passes apart,
against the host chain, and the LDS bank conflicts of its frame pass (profiles/spectrum.md).

28 streams x 5 s at 16 kHz, ``--n-fft`` 1024 at hop ``n_fft / 2``: two tones per stream over noise.

* (a) ``spectrum`` with the graph (three launches) and (b) without it (two), into preallocated
  outputs; (c) ``dst.copy_(src)`` of the audio's bytes; (d) the frame pass, (e) the reduce pass and
  (f) the graph pass alone, the library's entry points called as the operators call them, on the
  current stream; (g) (b) on a view one float off alignment, which the scalar frame pass serves.
  Device events around ``--iters`` back-to-back calls (one hipGraph of them, so that the host's
  launch time stays out) after 10 warm-ups, in ``--windows`` windows (median and spread reported).
* (h) the host chain on one core, per chunk of all streams: per stream ``np.fft.rfft`` of the Hann
  frames and the mean power's root (what ``PE_FFT`` would have to do for a framed spectrum), then the
  arithmetic of ``PE_AudioFilter``, ``PE_AudioResampler`` and ``render_xy``; host clock, ``--reps``
  repetitions, the median.  (i) ``spectrum_ref``, the definition, once.
* ``--pmc``: nothing is timed.  A fresh child process runs (b) a few times under ``rocprofv3 --pmc``
  with the LDS counters alone (no tracing next to them), and the frame pass's rows of the counter
  file are averaged.  The child's exit status is checked; a failure ends the script with it.

Usage:  python scripts/spectrum_bench.py [--pmc] [--out FILE.json]
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATE = 16000
COUNTERS = ("SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_INSTS_LDS", "SQ_WAVES")


def chunk(B, seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(seconds * RATE)
    t = np.arange(n, dtype=np.float64) / RATE
    rows = [0.5 * np.sin(2 * np.pi * (300.0 + 137.0 * b) * t) + 0.2 * np.sin(2 * np.pi * (2500.0 + 91.0 * b) * t) +
            0.02 * rng.standard_normal(n) for b in range(B)]
    return np.stack(rows).astype(np.float32)


def host_chain(x, n_fft, hop, kw, height, width):
    """What the host elements compute, for every stream of the chunk."""
    from aiko_services_amd.elements.media.audio_io import render_xy
    w = np.hanning(n_fft + 1)[:-1]
    w = w * (2.0 / w.sum())
    freq = np.fft.rfftfreq(n_fft, 1.0 / RATE)
    F = 1 + (x.shape[1] - n_fft) // hop
    idx = np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]
    images = []
    for row in x:
        a = np.sqrt((np.abs(np.fft.rfft(row[idx] * w, axis=-1)) ** 2).mean(axis=0))
        keep = (a >= kw["amplitude_minimum"]) & (a <= kw["amplitude_maximum"]) & (freq >= kw["frequency_minimum"]) & \
               (freq <= kw["frequency_maximum"])
        pa, pf = a[keep], freq[keep]
        order = np.argsort(-pa, kind="stable")[:kw["max_peaks"]]
        edges = np.linspace(0.0, kw["frequency_band_maximum"], kw["band_count"] + 1)
        band = np.searchsorted(edges, freq, side="right") - 1
        ok = (band >= 0) & (band < kw["band_count"])
        np.bincount(band[ok], weights=a[ok], minlength=kw["band_count"])
        images.append(render_xy(pf[order], pa[order], width, height, kw["frequency_maximum"], kw["amplitude_maximum"]))
    return images


def pmc(args):
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="spectrum_pmc_")
    cmd = [rocprof, "--pmc", *COUNTERS, "-d", out, "-o", "run", "--output-format", "csv", "--", sys.executable,
           os.path.abspath(__file__), "--child", "--n-fft", str(args.n_fft)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-2000:])
        raise SystemExit(res.returncode)
    rows = {}
    for path in glob.glob(os.path.join(out, "**", "run_counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            kind = next((k for k in ("frames", "reduce") if f"spectrum_{k}_kernel" in r["Kernel_Name"]), None)
            if kind:
                rows.setdefault(kind, {}).setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    shutil.rmtree(out, ignore_errors=True)
    if "frames" not in rows:
        raise SystemExit("spectrum_bench: no spectrum_frames_kernel rows in the counter file")
    result = {"pmc": {kind: {**{k: round(statistics.mean(v), 1) for k, v in sorted(c.items())},
                             "dispatches": len(next(iter(c.values())))} for kind, c in rows.items()}}
    print(json.dumps(result), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--streams", type=int, default=28)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--child", action="store_true", help="the run under the profiler: a few steps, nothing timed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.pmc:
        result = pmc(a)
    else:
        result = measure(a)
    if a.out and result is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


def measure(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spectrum_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd import ops
    from aiko_services_amd.ops import spectrum as S
    from aiko_services_amd.ops.reference import spectrum_graph_ref, spectrum_ref
    from scripts.yuv_bench import timed
    ops.require_native()
    B, n_fft, hop = a.streams, a.n_fft, a.n_fft // 2
    kw = {**S.DEFAULTS, "n_fft": n_fft, "hop": hop}
    gk = dict(height=480, width=640)
    host = chunk(B, a.seconds, 7)
    audio = torch.from_numpy(host).cuda()
    n = audio.shape[1]
    F, K = S.frame_count(n, n_fft, hop), n_fft // 2 + 1
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")  # noqa: E731
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="cuda")  # noqa: E731
    outs = dict(amplitudes=f32(B, K), band_amplitudes=f32(B, kw["band_count"]), peak_bins=i32(B, kw["max_peaks"]),
                peak_amplitudes=f32(B, kw["max_peaks"]), peak_counts=i32(B), power=f32(B, F, K))
    image = torch.empty(B, gk["height"], gk["width"], 3, dtype=torch.uint8, device="cuda")
    if a.child:
        for _ in range(5):
            S.spectrum(audio, **kw, **outs)
        torch.cuda.synchronize()
        return None
    names = ("amplitudes", "band_amplitudes", "peak_bins", "peak_amplitudes", "peak_counts", "power")
    ta = timed(lambda: S.spectrum(audio, graph=gk, image=image, **kw, **outs), a.iters, a.windows)
    tb = timed(lambda: S.spectrum(audio, **kw, **outs), a.iters, a.windows)
    want = [outs[k].clone() for k in names]
    src = torch.empty(audio.numel() * 2, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    tc = timed(lambda: dst.copy_(src), a.iters, a.windows)              # reads half, writes half: audio's bytes in all
    lib = ctypes.CDLL(str(ops._LIB))
    lib.aiko_spectrum_graph.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_double] + \
        [ctypes.c_int] * 3 + [ctypes.c_void_p]
    lib.aiko_spectrum_frames.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_long] + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p]
    lib.aiko_spectrum_reduce.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int] * 5 + [ctypes.c_float] * 3 + \
        [ctypes.c_int] * 3 + [ctypes.c_void_p]
    key = (float(kw["sample_rate"]), n_fft, kw["window"], kw["band_count"], float(kw["frequency_band_maximum"]),
           float(kw["amplitude_minimum"]), float(kw["amplitude_maximum"]), float(kw["frequency_minimum"]),
           float(kw["frequency_maximum"]))
    t = S.tables(*key)
    w, tw, band_start = S._device_tables(key, audio.device)
    bin_px = S._device_bin_px(n_fft, float(kw["sample_rate"]), float(kw["frequency_maximum"]), gk["width"], audio.device)
    p = lambda x: x.data_ptr()  # noqa: E731
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def frames():
        rc = lib.aiko_spectrum_frames(p(audio), p(w), p(tw), p(outs["power"]), B, n, F, n_fft, hop, stream())
        assert rc == 0, rc

    def reduce():
        rc = lib.aiko_spectrum_reduce(p(outs["power"]), p(band_start), p(outs["amplitudes"]), p(outs["band_amplitudes"]),
                                      p(outs["peak_bins"]), p(outs["peak_amplitudes"]), p(outs["peak_counts"]), B, F,
                                      n_fft, kw["band_count"], kw["max_peaks"], float(np.float32(1.0 / F)), t.lo, t.hi,
                                      t.k_lo, t.k_hi, 0, stream())
        assert rc == 0, rc

    def graph():
        rc = lib.aiko_spectrum_graph(p(outs["peak_bins"]), p(outs["peak_amplitudes"]), p(outs["peak_counts"]), p(bin_px),
                                     p(image), B, gk["height"], gk["width"], K, kw["max_peaks"],
                                     float(kw["amplitude_maximum"]), 0, 255, 0, stream())
        assert rc == 0, rc

    td, te, tf = (timed(fn, a.iters, a.windows) for fn in (frames, reduce, graph))
    flat = torch.empty(audio.numel() + 4, dtype=torch.float32, device="cuda")
    off = flat[1:1 + audio.numel()].view(audio.shape)
    off.copy_(audio)
    assert not S.spectrum_uses_vector(off, hop) and S.spectrum_uses_vector(audio, hop)
    tg = timed(lambda: S.spectrum(off, **kw, **outs), a.iters, a.windows)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[k], w_) for k, w_ in zip(names, want)), "scalar pass differs from the vector pass"
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        host_chain(host, n_fft, hop, kw, gk["height"], gk["width"])
        times.append((time.perf_counter() - t0) * 1e3)
    th = statistics.median(times)
    t0 = time.perf_counter()
    ref = spectrum_ref(torch.from_numpy(host), **kw)
    ref_image = spectrum_graph_ref(ref[2], ref[3], ref[4], n_fft=n_fft, x_max=kw["frequency_maximum"],
                                   y_max=kw["amplitude_maximum"], **gk)
    ti = (time.perf_counter() - t0) * 1e3
    assert all(torch.equal(outs[k].cpu(), r) for k, r in zip(names, ref)), "kernels differ from the reference"
    assert torch.equal(image.cpu(), ref_image), "graph differs from the reference"
    row = {"streams": B, "seconds": a.seconds, "n_fft": n_fft, "hop": hop, "F": F, "bytes_audio": audio.numel() * 4,
           "bytes_power": outs["power"].numel() * 4, "bytes_image": image.numel(), "peaks": ref[4].tolist(),
           "a_spectrum_with_graph": ta, "b_spectrum": tb, "c_copy_audio_bytes": tc, "d_frame_pass": td,
           "e_reduce_pass": te, "f_graph_pass": tf, "g_scalar_step": tg,
           "d_over_c": round(td["median_us"] / tc["median_us"], 2), "h_host_chain_ms": round(th, 1),
           "h_over_a": round(th * 1e3 / ta["median_us"]), "i_reference_ms": round(ti, 1)}
    print(json.dumps(row), flush=True)
    return {"rows": [row]}


if __name__ == "__main__":
    main()
