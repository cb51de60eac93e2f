"""voice_activity at the Whisper bench shapes against a plain copy of the same bytes, its two passes
apart, against the CPU reference, and what the decoder's gate saves (profiles/vad.md).

Two shapes: 28 streams x 5 s chunks (the Whisper bench's) and 1 stream x 30 s, at ``--frame``
samples per frame; noise at 0.02 with a 0.3 tone in the middle third of every chunk, so that the
stream pass walks real runs.

* (a) ``voice_activity`` into preallocated outputs; (b) ``dst.copy_(src)`` of the audio's bytes, the
  roof of the frame pass; (c) the frame pass alone and (d) the stream pass alone, the library's two
  entry points called as ``voice_activity_out`` calls them, on the current stream; (e) (a) on a view
  one float off alignment, which the scalar frame pass serves.  Device events around ``--iters``
  back-to-back calls (one hipGraph of them, so that the host's launch time stays out) after 10
  warm-ups, in ``--windows`` windows (median and spread reported).
* (f) ``voice_activity_ref`` on the same chunk on one host core, host clock, one repetition.
* ``--decoder``: ``WhisperDecoder.transcribe`` of whisper-``--size`` on random features of 28 streams
  x 30 s, 96 new tokens, stop_early every 8 steps, with ``silent`` absent (the call as it was before
  the gate existed), all zeros, half ones and all ones: host clock around the call, device
  synchronised, ``--reps`` repetitions after a warm-up, the four alternating.

Usage:  python scripts/vad_bench.py [--decoder] [--out FILE.json]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.yuv_bench import timed  # noqa: E402

RATE = 16000


def chunk(B, seconds, seed):
    g = torch.Generator().manual_seed(seed)
    n = int(seconds * RATE)
    t = torch.arange(n, dtype=torch.float64) / RATE
    x = 0.02 * torch.randn(B, n, generator=g)
    x[:, n // 3:2 * n // 3] += (0.3 * torch.sin(2 * math.pi * 440.0 * t[n // 3:2 * n // 3])).float()
    return x.contiguous()


def passes(lib, audio, state, outs, kw):
    """The two launches of one step as separate callables."""
    B, n = audio.shape
    frame = kw["frame"]
    F = n // frame
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

    def frames():
        rc = lib.aiko_vad_frames(p(audio), p(outs["level"]), p(outs["zc"]), B, F, frame, stream())
        assert rc == 0, rc

    def stream_pass():
        rc = lib.aiko_vad_stream(p(outs["level"]), p(outs["zc"]), p(state.v), p(outs["state_out"].v), p(outs["mask"]),
                                 p(outs["seg"]), p(outs["count"]), p(outs["speech"]), p(outs["silent"]), B, F, frame,
                                 kw["threshold"], kw["min_level"], kw["up_shift"], kw["speech_shift"],
                                 kw["down_shift"], kw["warmup"], kw["attack"], kw["hang"], kw["max_zc"], kw["window"],
                                 kw["max_seg"], stream())
        assert rc == 0, rc

    return frames, stream_pass


def decoder_rows(size, reps):
    from aiko_services_amd.models.whisper_decoder import WhisperDecoder
    B, T = 28, 1500
    dec = WhisperDecoder(size, device=torch.device("cuda"))
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(B, T + 1, dec.d, generator=g).to("cuda", torch.bfloat16)[:, :T]
    half = torch.zeros(B, dtype=torch.int32, device="cuda")
    half[::2] = 1
    cases = {"ungated": None, "none_silent": torch.zeros_like(half), "half_silent": half,
             "all_silent": torch.ones_like(half)}
    times = {k: [] for k in cases}
    steps = {}
    dec.transcribe(feats, max_new_tokens=96)
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, silent in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tok = dec.transcribe(feats, max_new_tokens=96, check_every=8, silent=silent)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            steps[name] = tok.shape[1] - 1
    return {name: {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2),
                   "max_ms": round(max(v), 2), "steps": steps[name]} for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", type=int, default=320)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--decoder", action="store_true")
    ap.add_argument("--size", default="small")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vad_bench: needs a GPU (nothing is measured on the CPU)")
    from aiko_services_amd import ops
    from aiko_services_amd.ops import vad as V
    from aiko_services_amd.ops.reference import voice_activity_ref
    ops.require_native()
    lib = ctypes.CDLL(str(ops._LIB))
    kw = dict(V.DEFAULTS, frame=a.frame)
    rows = []
    for B, seconds in ((28, 5.0), (1, 30.0)):
        host = chunk(B, seconds, 10 * B)
        audio = host.cuda()
        F = audio.shape[1] // a.frame
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device="cuda")  # noqa: E731
        # a state past the warm-up, as a stream in service has it
        state = V.voice_activity(audio, V.new_state(B, "cuda"), **kw)[7]
        outs = dict(mask=torch.empty(B, F, dtype=torch.uint8, device="cuda"), seg=i32(B, kw["max_seg"], 2),
                    count=i32(B), speech=i32(B), silent=i32(B), level=i32(B, F), zc=i32(B, F),
                    state_out=V.VadState(i32(B, 8)))
        ta = timed(lambda: V.voice_activity(audio, state, **outs, **kw), a.iters, a.windows)
        want = [t.clone() for t in (*[outs[k] for k in ("mask", "seg", "count", "speech", "silent", "level", "zc")],
                                    outs["state_out"].v)]
        src = torch.empty(audio.numel() * 2, dtype=torch.uint8, device="cuda").random_(0, 256)
        dst = torch.empty_like(src)
        tb = timed(lambda: dst.copy_(src), a.iters, a.windows)          # reads half, writes half: audio's bytes in all
        frames, stream_pass = passes(lib, audio, state, outs, kw)
        tc = timed(frames, a.iters, a.windows)
        td = timed(stream_pass, a.iters, a.windows)
        flat = torch.empty(audio.numel() + 4, dtype=torch.float32, device="cuda")
        off = flat[1:1 + audio.numel()].view(audio.shape)
        off.copy_(audio)
        assert not V.vad_uses_vector(off) and V.vad_uses_vector(audio)
        te = timed(lambda: V.voice_activity(off, state, **outs, **kw), a.iters, a.windows)
        torch.cuda.synchronize()
        got = [*[outs[k] for k in ("mask", "seg", "count", "speech", "silent", "level", "zc")], outs["state_out"].v]
        assert all(torch.equal(g_, w) for g_, w in zip(got, want)), "scalar pass differs from the vector pass"
        cpu_state = V.VadState(state.v.cpu())
        t0 = time.perf_counter()
        ref = voice_activity_ref(host, cpu_state, **kw)
        tf = (time.perf_counter() - t0) * 1e3
        assert all(torch.equal(g_.cpu(), w) for g_, w in zip(got, (*ref[:7], ref[7].v))), "kernels differ from the reference"
        rows.append({"streams": B, "seconds": seconds, "frame": a.frame, "F": F, "bytes_audio": audio.numel() * 4,
                     "grid_frames": V.frame_grid(F, B), "speech_frames": int(ref[3].sum()),
                     "segments": int(ref[2].sum()), "a_voice_activity": ta, "b_copy_audio_bytes": tb,
                     "c_frame_pass": tc, "d_stream_pass": td, "e_scalar_step": te,
                     "c_over_b": round(tc["median_us"] / tb["median_us"], 2), "f_reference_ms": round(tf, 1),
                     "f_over_a": round(tf * 1e3 / ta["median_us"])})
        print(json.dumps(rows[-1]), flush=True)
    result = {"rows": rows}
    if a.decoder:
        result["decoder"] = decoder_rows(a.size, a.reps)
        print(json.dumps(result["decoder"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
