"""Audio front end ops (``csrc/kernels/audio_ops.hip``): Whisper log-mel spectrogram.

``mel_filters`` builds the Slaney-style mel filterbank (the librosa default Whisper ships as
``mel_filters.npz``; computed here since no assets are available offline).

Raw PCM in (``csrc/kernels/resample_ops.hip``): :func:`resample` downmixes interleaved int16 or
fp32 PCM to mono and converts its sample rate with a Kaiser-windowed sinc polyphase filter
(:func:`resample_filter`), one launch per chunk, the stream's last ``T-1`` samples carried in
``hist``.  The arithmetic, all fp32, in exactly this order, no operation fused with another::

    mono, int16:  float(int32 sum of the C samples) * float32(1/(32768*C))
    mono, fp32:   ((x0 + x1) + ...) * float32(1/C)
    s[b]        = hist[b] ++ mono[b]                      (T-1+n_in samples)
    i0 = (j*M)//L ;  p = (j*M)%L
    out[b][j]   = acc after  acc = 0; for k = 0..T-1: acc = acc + filt[p][k]*s[b][i0+k]
    hist_out[b] = s[b][n_in : n_in+T-1]

:func:`~aiko_services_amd.ops.reference.resample_ref` is the same on the CPU, bit for bit."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

SAMPLE_RATE = 16000
N_FFT = 400
HOP = 160

__all__ = ["mel_filters", "log_mel", "log_mel_ref", "SAMPLE_RATE", "N_FFT", "HOP", "RESAMPLE_CHAINS",
           "RESAMPLE_MAX_LDS", "RESAMPLE_MAX_TAPS", "RESAMPLE_THREADS", "RESAMPLE_TILE", "resample", "resample_delay",
           "resample_filter", "resample_grid", "resample_lds_bytes", "resample_uses_vector"]


def _hz_to_mel(f):
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return f / f_sp if f < min_log_hz else min_log_mel + math.log(f / min_log_hz) / logstep


def _mel_to_hz(m: torch.Tensor) -> torch.Tensor:
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return torch.where(m >= min_log_mel, min_log_hz * torch.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filters(n_mels: int = 80, n_fft: int = N_FFT, sr: int = SAMPLE_RATE) -> torch.Tensor:
    """[n_mels, n_fft // 2 + 1] fp32 Slaney mel filterbank (area-normalised triangles)."""
    fft_freqs = torch.linspace(0, sr / 2, n_fft // 2 + 1, dtype=torch.float64)
    mels = torch.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2), n_mels + 2, dtype=torch.float64)
    mel_f = _mel_to_hz(mels)
    fdiff = mel_f[1:] - mel_f[:-1]
    ramps = mel_f[:, None] - fft_freqs[None, :]
    w = torch.zeros(n_mels, n_fft // 2 + 1, dtype=torch.float64)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = torch.clamp(torch.minimum(lower, upper), min=0)
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    return (w * enorm[:, None]).float()


_RANGES: dict = {}


def mel_ranges(filters: torch.Tensor) -> torch.Tensor:
    """int32 [n_mels, 3] = (first nonzero bin, run length, offset into the packed weights) of
    each triangular filter — the log-mel kernel's sparse filterbank (cached per tensor)."""
    key = (filters.data_ptr(), filters._version, tuple(filters.shape))
    r = _RANGES.get(key)
    if r is None:
        rows, off = [], 0
        for w in filters.detach().float().cpu():
            nz = torch.nonzero(w != 0).flatten()
            lo = int(nz[0]) if nz.numel() else 0
            n = int(nz[-1]) - lo + 1 if nz.numel() else 0
            rows.append((lo, n, off))
            off += n
        if off > 2048:
            raise ValueError(f"mel filterbank has {off} nonzero span elements (kernel limit 2048)")
        r = _RANGES[key] = torch.tensor(rows, dtype=torch.int32, device=filters.device)
    return r


def log_mel(audio: torch.Tensor, filters: torch.Tensor, out: torch.Tensor, rows: int, pad: int,
            work: torch.Tensor | None = None, gmax: torch.Tensor | None = None, frames: int | None = None):
    """fp32 audio [B, N] -> Whisper-normalised log-mel, bf16, frame t of clip b at row
    ``b*rows + pad + t`` of ``out`` [B*rows, n_mels] (other rows zero: conv padding)."""
    B, N = audio.shape
    F = frames if frames is not None else N // HOP
    n_mels = filters.shape[0]
    if work is None:
        work = torch.empty(B * F * n_mels, dtype=torch.float32, device=audio.device)
    if gmax is None:
        gmax = torch.empty(B, dtype=torch.int32, device=audio.device)
    torch.ops.aiko.logmel_out(audio, filters, mel_ranges(filters), N_FFT, HOP, F, work, gmax, out, rows, pad)
    return out


def log_mel_ref(audio: torch.Tensor, filters: torch.Tensor, frames: int | None = None) -> torch.Tensor:
    """Whisper's reference log-mel (torch.stft), fp32 [B, n_mels, F]."""
    window = torch.hann_window(N_FFT, device=audio.device)
    stft = torch.stft(audio, N_FFT, HOP, window=window, return_complex=True)
    mag = stft[..., :-1].abs() ** 2
    if frames is not None:
        mag = mag[..., :frames]
    mel = filters.to(audio.device) @ mag
    log_spec = torch.clamp(mel, min=1e-10).log10()
    log_spec = torch.maximum(log_spec, log_spec.amax(dim=(1, 2), keepdim=True) - 8.0)
    return (log_spec + 4.0) / 4.0


def window_shift(src: torch.Tensor, chunk: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """``dst[b] = concat(src[b, n:], chunk[b])`` — a sliding audio window advanced by one chunk
    (fp32 [B, W] / [B, n]); one HIP kernel on the GPU, torch slicing on the CPU."""
    n = chunk.shape[1]
    if dst.is_cuda:
        torch.ops.aiko.window_shift_out(src, chunk, dst)
    else:
        dst[:, :dst.shape[1] - n].copy_(src[:, n:])
        dst[:, dst.shape[1] - n:].copy_(chunk)
    return dst


# ---- raw PCM in: downmix + polyphase sample-rate conversion (csrc/kernels/resample_ops.hip) ----

# the kernel's tiling (resample_ops.hip: RS_THREADS, RS_CHAINS, RS_TILE, RS_MAX_TAPS, RS_MAX_LDS)
RESAMPLE_THREADS = 256       # threads of a workgroup
RESAMPLE_CHAINS = 4          # independent outputs of a thread
RESAMPLE_TILE = RESAMPLE_THREADS * RESAMPLE_CHAINS      # consecutive outputs of a workgroup
RESAMPLE_MAX_TAPS = 16384    # L*T: 64 KiB of taps
RESAMPLE_MAX_LDS = 160 * 1024


def resample_lds_bytes(L: int, M: int, T: int) -> int:
    """LDS of a workgroup: the ``L*T`` taps and the most samples a tile's outputs read."""
    return 4 * (L * T + ((RESAMPLE_TILE - 1) * M + L - 1) // L + T)


@functools.lru_cache(maxsize=64)
def resample_filter(rate_in: int, rate_out: int, zeros: int = 16, beta: float = 9.0, rolloff: float = 0.9):
    """``(filt, L, M)``: the polyphase taps, fp32 ``[L, T]`` on the CPU, of a Kaiser-windowed sinc
    low-pass for ``rate_in`` -> ``rate_out``, with ``L / M = rate_out / rate_in`` in lowest terms.
    The cutoff is ``rolloff`` times the lower Nyquist frequency, the window spans ``zeros`` zero
    crossings of the sinc on each side (``T = 2*ceil(zeros * max(1, M/L))`` taps per phase), every
    row sums to 1.  Equal rates give ``[[1.0]]``.  The output lags the input by ``T/2`` input samples
    (:func:`resample_delay`).

    ``ValueError`` when ``L*T > 16384`` (64 KiB of taps: a workgroup keeps the table in LDS) —
    11025 Hz -> 16 kHz (L = 640, T = 32) is refused by this rule — or when the taps and the samples
    of one tile of outputs exceed the 160 KiB of LDS (decimation by 38 or more).  Cached: the same
    arguments return the same tensor, which callers must not modify."""
    rate_in, rate_out, zeros = int(rate_in), int(rate_out), int(zeros)
    if rate_in < 1 or rate_out < 1 or zeros < 1 or not 0.0 < rolloff <= 1.0 or beta < 0:
        raise ValueError(f"resample_filter: bad arguments {(rate_in, rate_out, zeros, beta, rolloff)}")
    g = math.gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    if L == M:
        return torch.ones(1, 1, dtype=torch.float32), 1, 1
    fc = min(1.0, L / M) * rolloff
    T = 2 * math.ceil(zeros * max(1.0, M / L))
    if L * T > RESAMPLE_MAX_TAPS:
        raise ValueError(f"resample_filter: {rate_in} -> {rate_out} Hz needs L*T = {L}*{T} = {L * T} taps, "
                         f"more than {RESAMPLE_MAX_TAPS}")
    if resample_lds_bytes(L, M, T) > RESAMPLE_MAX_LDS:
        raise ValueError(f"resample_filter: {rate_in} -> {rate_out} Hz needs {resample_lds_bytes(L, M, T)} bytes of "
                         f"LDS per workgroup, more than {RESAMPLE_MAX_LDS}")
    p = np.arange(L, dtype=np.float64)[:, None]
    k = np.arange(T, dtype=np.float64)[None, :]
    tau = p / L + (T / 2 - 1) - k
    window = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (2.0 * tau / T) ** 2))) / np.i0(beta)
    h = fc * np.sinc(fc * tau) * window
    h = h / h.sum(axis=1, keepdims=True)
    return torch.from_numpy(h.astype(np.float32)), L, M


def resample_delay(rate_in: int, rate_out: int, zeros: int = 16, beta: float = 9.0, rolloff: float = 0.9) -> float:
    """Seconds by which :func:`resample`'s output lags its input: ``T/2`` input samples (1 ms for
    48 kHz -> 16 kHz), 0 for equal rates."""
    filt, _, _ = resample_filter(rate_in, rate_out, zeros, beta, rolloff)
    T = filt.shape[1]
    return 0.0 if T == 1 else (T / 2) / float(rate_in)


def resample_uses_vector(pcm: torch.Tensor) -> bool:
    """Whether the vector kernel serves this ``pcm`` ``[B, n_in, C]``: mono or stereo, 16-byte
    aligned, a stream's row a multiple of 16 bytes (every 16-byte load then holds whole frames of
    one stream); every other call runs the scalar kernel."""
    return pcm.shape[2] <= 2 and pcm.data_ptr() % 16 == 0 and \
        (pcm.shape[1] * pcm.shape[2] * pcm.element_size()) % 16 == 0


def resample_grid(n_out: int, batch: int) -> tuple[int, int]:
    """The launch's grid: ``ceil(n_out / RESAMPLE_TILE)`` tiles of outputs and one workgroup for
    ``hist_out`` per stream, times ``batch`` streams."""
    return (int(n_out) + RESAMPLE_TILE - 1) // RESAMPLE_TILE + 1, int(batch)


def resample(pcm: torch.Tensor, hist: torch.Tensor, filt: torch.Tensor, L: int, M: int,
             out: torch.Tensor | None = None, hist_out: torch.Tensor | None = None):
    """Device ``pcm`` ``[B, n_in, C]`` (contiguous, int16 or fp32, ``1 <= C <= 8``), the ``T-1`` mono
    samples before it ``hist`` fp32 ``[B, T-1]`` (zeros at the start of a stream) and ``filt`` fp32
    ``[L, T]`` on the device -> ``(out, hist_out)``: fp32 ``[B, n_in*L/M]`` and the history of the
    next chunk ``[B, T-1]``.  ``n_in*L % M == 0`` is required, so every chunk starts at phase 0.
    One launch, no synchronisation, no allocation when ``out`` and ``hist_out`` are given.
    ``hist_out`` must not overlap ``hist`` or ``pcm``; by default both outputs are new."""
    L, M = int(L), int(M)
    if out is None or hist_out is None:
        if pcm.dim() != 3:
            raise ValueError(f"resample: pcm [B, n_in, C] required, got {tuple(pcm.shape)}")
        if L < 1 or M < 1 or (pcm.shape[1] * L) % M:
            raise ValueError(f"resample: n_in*L % M != 0 for n_in = {pcm.shape[1]}, L / M = {L} / {M}")
        if out is None:
            out = torch.empty(pcm.shape[0], pcm.shape[1] * L // M, dtype=torch.float32, device=pcm.device)
        if hist_out is None:
            hist_out = torch.empty_like(hist)
    torch.ops.aiko.resample_out(pcm, hist, filt, L, M, out, hist_out)
    return out, hist_out
