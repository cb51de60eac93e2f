// Whisper front end for gfx950: log-mel spectrogram of 16 kHz audio, fully on the GPU.
//
// logmel_kernel: one 256-thread workgroup per 16 STFT frames of one clip.  Frames (n_fft 400,
// hop 160, centred with reflect padding, periodic Hann window) are staged in LDS; the 201-bin
// power spectrum is a direct DFT against an LDS twiddle table (0.26 MFLOP per frame: a few
// microseconds for a 30 s clip, not worth an FFT's passes at this size); the mel filterbank
// maps it to mel energies — sparse: each triangular filter covers a contiguous bin range
// (host-computed lo / len / offset), whose weights (~400 nonzeros of 80 x 201) are staged in
// LDS per workgroup (the dense 201-term dot per (frame, mel) from L2 took most of the former
// 522 us per 16-clip batch); log10(max(e, 1e-10)) is written and the clip's maximum is kept
// with an order-preserving integer atomicMax.
// logmel_finalize_kernel: Whisper's dynamic-range clamp max(x, max - 8), (x + 4) / 4, written
// as bf16 straight into the zero-bordered [rows][80] buffer the first conv reads.
#include <cstdlib>

#include "common.h"
#include "aiko_api.h"

namespace aiko {

constexpr int kFPB = 16;         // frames per workgroup
constexpr int kMaxFFT = 400;
constexpr int kMaxBins = kMaxFFT / 2 + 1;

__device__ __forceinline__ int float_order_key(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float float_from_key(int k) {
  return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff);
}

constexpr int kMaxMels = 128;
constexpr int kMaxMelNnz = 2048;

__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ audio, int N,
                                                      const float* __restrict__ mel, int n_mels,
                                                      const int* __restrict__ mel_range,
                                                      int n_fft, int hop, int F,
                                                      float* __restrict__ out, int* __restrict__ gmax) {
  __shared__ float tw_c[kMaxFFT], tw_s[kMaxFFT];
  __shared__ float frame[kFPB][kMaxFFT];
  __shared__ float power[kFPB][kMaxBins];
  __shared__ float mw[kMaxMelNnz];
  __shared__ int mr[kMaxMels][3];               // lo bin, length, offset into mw
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * kFPB;
  const int nbins = n_fft / 2 + 1;
  const float* x = audio + (long)b * N;
  for (int i = tid; i < n_mels * 3; i += 256) mr[i / 3][i % 3] = mel_range[i];
  __syncthreads();
  for (int m = tid >> 4; m < n_mels; m += 16) {           // 16 lanes per filter row
    const int lo = mr[m][0], len = mr[m][1], off = mr[m][2];
    for (int j = tid & 15; j < len; j += 16) mw[off + j] = mel[(long)m * nbins + lo + j];
  }
  for (int n = tid; n < n_fft; n += 256) {
    float s, c;
    sincosf(6.283185307179586f * n / n_fft, &s, &c);
    tw_c[n] = c;
    tw_s[n] = s;
  }
  for (int i = tid; i < kFPB * n_fft; i += 256) {
    const int f = i / n_fft, n = i - f * n_fft;
    float v = 0.f;
    if (f0 + f < F) {
      int idx = (f0 + f) * hop - n_fft / 2 + n;
      if (idx < 0) idx = -idx;
      if (idx >= N) idx = 2 * (N - 1) - idx;
      const float w = 0.5f - 0.5f * cospif(2.f * n / n_fft);
      v = x[idx] * w;
    }
    frame[f][n] = v;
  }
  __syncthreads();
  // one thread per frequency bin, all kFPB frames at once: each twiddle gather from LDS feeds
  // 2 * kFPB FMAs and the frame samples are wave-wide broadcasts
  for (int k = tid; k < nbins; k += 256) {
    float re[kFPB], im[kFPB];
#pragma unroll
    for (int f = 0; f < kFPB; ++f) re[f] = im[f] = 0.f;
    int t = 0;
    for (int n = 0; n < n_fft; ++n) {
      const float c = tw_c[t], sn = tw_s[t];
#pragma unroll
      for (int f = 0; f < kFPB; ++f) {
        const float v = frame[f][n];
        re[f] += v * c;
        im[f] -= v * sn;
      }
      t += k;
      if (t >= n_fft) t -= n_fft;
    }
#pragma unroll
    for (int f = 0; f < kFPB; ++f) power[f][k] = re[f] * re[f] + im[f] * im[f];
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int pr = tid; pr < kFPB * n_mels; pr += 256) {
    const int f = pr / n_mels, m = pr - f * n_mels;
    if (f0 + f >= F) continue;
    const int lo = mr[m][0], len = mr[m][1], off = mr[m][2];
    float e = 0.f;
    for (int j = 0; j < len; ++j) e += mw[off + j] * power[f][lo + j];
    const float l = log10f(fmaxf(e, 1e-10f));
    out[((long)b * F + f0 + f) * n_mels + m] = l;
    mx = fmaxf(mx, l);
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(gmax + b, float_order_key(m));
  }
}

// ---------------------------------------------------------------------------------------------
// Whisper's n_fft = 400 as a real FFT: the 400 windowed samples of a frame are packed as 200
// complex points z[n] = x[2n] + i x[2n+1], transformed by a mixed-radix (2 x 4 x 5 x 5)
// Stockham FFT in LDS (each stage reads one buffer, writes the other in natural order), and
// split into the 201 bins of the real transform: X[k] = E[k] + W400^k O[k] with
// E = (Z[k] + conj Z[200-k]) / 2, O = -i (Z[k] - conj Z[200-k]) / 2.  ~10 kFLOP per frame
// instead of the direct DFT's 160 kFLOP (measured 465 us per 16-clip batch with the DFT).
constexpr int kHalf = 200;

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

template <int R>
__device__ __forceinline__ void small_dft(float2 (&v)[R]) {
  if constexpr (R == 2) {
    const float2 a = v[0], b = v[1];
    v[0] = make_float2(a.x + b.x, a.y + b.y);
    v[1] = make_float2(a.x - b.x, a.y - b.y);
  } else if constexpr (R == 4) {
    const float2 t0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y);
    const float2 t1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
    const float2 t2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y);
    const float2 d = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
    const float2 t3 = make_float2(d.y, -d.x);                       // -i * d
    v[0] = make_float2(t0.x + t2.x, t0.y + t2.y);
    v[2] = make_float2(t0.x - t2.x, t0.y - t2.y);
    v[1] = make_float2(t1.x + t3.x, t1.y + t3.y);
    v[3] = make_float2(t1.x - t3.x, t1.y - t3.y);
  } else {                                                          // R == 5, direct
    const float c1 = 0.30901699437494745f, c2 = -0.8090169943749473f;
    const float s1 = 0.9510565162951535f, s2 = 0.5877852522924732f;
    const float2 w[5] = {make_float2(1.f, 0.f), make_float2(c1, -s1), make_float2(c2, -s2),
                         make_float2(c2, s2), make_float2(c1, s1)};
    float2 out[5];
#pragma unroll
    for (int u = 0; u < 5; ++u) {
      float2 acc = v[0];
#pragma unroll
      for (int q = 1; q < 5; ++q) {
        const float2 t = cmul(v[q], w[(u * q) % 5]);
        acc.x += t.x;
        acc.y += t.y;
      }
      out[u] = acc;
    }
#pragma unroll
    for (int u = 0; u < 5; ++u) v[u] = out[u];
  }
}

// one Stockham stage of radix R over kFPB frames: buffers [kFPB][kHalf]
template <int R>
__device__ __forceinline__ void fft_stage(const float2 (*in)[kHalf], float2 (*out)[kHalf], int Ns,
                                          const float* tw_c, const float* tw_s) {
  constexpr int M = kHalf / R;
  for (int item = threadIdx.x; item < kFPB * M; item += 256) {
    const int f = item / M, j = item - f * M;
    const int jj = j % Ns;
    const int step = jj * (kHalf / (Ns * R));                       // W200^(q * step)
    float2 v[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      float2 a = in[f][j + q * M];
      if (q) {
        const int t = 2 * ((q * step) % kHalf);                     // W200^i = W400^(2i)
        a = cmul(a, make_float2(tw_c[t], -tw_s[t]));
      }
      v[q] = a;
    }
    small_dft<R>(v);
    const int dst = (j / Ns) * Ns * R + jj;
#pragma unroll
    for (int q = 0; q < R; ++q) out[f][dst + q * Ns] = v[q];
  }
  __syncthreads();
}

static_assert((kFPB - 1) * 160 + 400 <= kFPB * 201, "sample segment must fit the power buffer");
__global__ __launch_bounds__(256) void logmel_fft400_kernel(const float* __restrict__ audio, int N,
                                                             const float* __restrict__ mel, int n_mels,
                                                             const int* __restrict__ mel_range, int hop,
                                                             int F, float* __restrict__ out,
                                                             int* __restrict__ gmax) {
  constexpr int NFFT = 2 * kHalf, NB = kHalf + 1;
  __shared__ float tw_c[NFFT], tw_s[NFFT];
  __shared__ float2 buf0[kFPB][kHalf], buf1[kFPB][kHalf];
  __shared__ float power[kFPB][NB];
  __shared__ float mw[kMaxMelNnz];
  __shared__ int mr[kMaxMels][3];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * kFPB;
  const float* x = audio + (long)b * N;
  for (int n = tid; n < NFFT; n += 256) {
    float sn, c;
    sincosf(6.283185307179586f * n / NFFT, &sn, &c);
    tw_c[n] = c;
    tw_s[n] = sn;
  }
  for (int i = tid; i < n_mels * 3; i += 256) mr[i / 3][i % 3] = mel_range[i];
  // the 16 overlapping frames span one contiguous sample segment: stage it in LDS with all of a
  // thread's loads in flight at once (a load-per-sample loop pays one memory latency each),
  // reflect padding at the clip ends; periodic Hann window as a table
  float* seg = reinterpret_cast<float*>(&power[0][0]);             // power is not live yet
  constexpr int kSegMax = kFPB * NB;                                  // 3216 floats >= 15*hop+400
  const int seglen = (kFPB - 1) * hop + NFFT;
  const int s0 = f0 * hop - NFFT / 2;
  {
    float v[13];
#pragma unroll
    for (int u = 0; u < 13; ++u) {
      const int i = tid + u * 256;
      int idx = s0 + i;
      if (idx < 0) idx = -idx;
      if (idx >= N) idx = 2 * (N - 1) - idx;
      idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);
      v[u] = (i < seglen && i < kSegMax) ? x[idx] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 13; ++u) {
      const int i = tid + u * 256;
      if (i < seglen && i < kSegMax) seg[i] = v[u];
    }
  }
  float* win = reinterpret_cast<float*>(&buf1[0][0]);                // buf1 is not live yet
  for (int n = tid; n < NFFT; n += 256) win[n] = 0.5f - 0.5f * cospif(2.f * n / NFFT);
  __syncthreads();
  // windowed frames packed as complex pairs
  for (int i = tid; i < kFPB * kHalf; i += 256) {
    const int f = i / kHalf, n2 = i - f * kHalf;
    float2 v = make_float2(0.f, 0.f);
    if (f0 + f < F) {
      const int o = f * hop + 2 * n2;
      v = make_float2(seg[o] * win[2 * n2], seg[o + 1] * win[2 * n2 + 1]);
    }
    buf0[f][n2] = v;
  }
  __syncthreads();
  for (int m = tid >> 4; m < n_mels; m += 16) {
    const int lo = mr[m][0], len = mr[m][1], off = mr[m][2];
    for (int j = tid & 15; j < len; j += 16) mw[off + j] = mel[(long)m * NB + lo + j];
  }
  fft_stage<2>(buf0, buf1, 1, tw_c, tw_s);
  fft_stage<4>(buf1, buf0, 2, tw_c, tw_s);
  fft_stage<5>(buf0, buf1, 8, tw_c, tw_s);
  fft_stage<5>(buf1, buf0, 40, tw_c, tw_s);                          // Z in buf0, natural order
  for (int i = tid; i < kFPB * NB; i += 256) {
    const int f = i / NB, k = i - f * NB;
    const float2 zk = buf0[f][k % kHalf];
    const float2 zr = buf0[f][(kHalf - k) % kHalf];
    const float2 ev = make_float2(0.5f * (zk.x + zr.x), 0.5f * (zk.y - zr.y));   // (Zk + conj Zr) / 2
    const float2 od = make_float2(0.5f * (zk.y + zr.y), -0.5f * (zk.x - zr.x));  // -i (Zk - conj Zr) / 2
    const float2 t = cmul(od, make_float2(tw_c[k], -tw_s[k]));
    const float re = ev.x + t.x, im = ev.y + t.y;
    power[f][k] = re * re + im * im;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int pr = tid; pr < kFPB * n_mels; pr += 256) {
    const int f = pr / n_mels, m = pr - f * n_mels;
    if (f0 + f >= F) continue;
    const int lo = mr[m][0], len = mr[m][1], off = mr[m][2];
    float e = 0.f;
    for (int j = 0; j < len; ++j) e += mw[off + j] * power[f][lo + j];
    const float l = log10f(fmaxf(e, 1e-10f));
    out[((long)b * F + f0 + f) * n_mels + m] = l;
    mx = fmaxf(mx, l);
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(gmax + b, float_order_key(m));
  }
}

// dst rows per clip = rows (>= F + pad + pad_end); frame t of clip b -> row b*rows + pad + t
__global__ void logmel_finalize_kernel(const float* __restrict__ logmel, const int* __restrict__ gmax,
                                       bf16_t* __restrict__ dst, int B, int F, int n_mels, int rows,
                                       int pad, int ld) {
  const long total = (long)B * rows * n_mels;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int m = i % n_mels;
    const long r = i / n_mels;
    const int b = r / rows, row = r - (long)b * rows;
    const int t = row - pad;
    float y = 0.f;
    if (t >= 0 && t < F) {
      const float mx = float_from_key(gmax[b]);
      y = (fmaxf(logmel[((long)b * F + t) * n_mels + m], mx - 8.f) + 4.f) * 0.25f;
    }
    dst[((long)b * rows + row) * ld + m] = f2bf(y);
  }
}

// Same, 8 mels per thread (n_mels % 8 == 0, 16-byte aligned rows): two float4 loads, one 16-byte
// store of 8 bf16 and 32-bit index math -- the scalar version does a 64-bit division and a 2-byte
// store per element.  Identical per-element arithmetic and rounding.
__global__ __launch_bounds__(256) void logmel_finalize8_kernel(const float* __restrict__ logmel,
                                                               const int* __restrict__ gmax,
                                                               bf16_t* __restrict__ dst, int B, int F,
                                                               int n_mels, int rows, int pad, int ld) {
  const int n8 = n_mels >> 3;
  const int total = B * rows * n8;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int r = i / n8, m8 = i - r * n8;
    const int b = r / rows, row = r - b * rows;
    const int t = row - pad;
    u32x4 o = {0u, 0u, 0u, 0u};
    if (t >= 0 && t < F) {
      const float mx = float_from_key(gmax[b]) - 8.f;
      const f32x4* src = reinterpret_cast<const f32x4*>(logmel + ((long)b * F + t) * n_mels + m8 * 8);
      const f32x4 u0 = src[0], u1 = src[1];
      const float v[8] = {u0[0], u0[1], u0[2], u0[3], u1[0], u1[1], u1[2], u1[3]};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned lo = f2bf((fmaxf(v[2 * e], mx) + 4.f) * 0.25f);
        const unsigned hi = f2bf((fmaxf(v[2 * e + 1], mx) + 4.f) * 0.25f);
        o[e] = lo | (hi << 16);
      }
    }
    *reinterpret_cast<u32x4*>(dst + ((long)b * rows + row) * ld + m8 * 8) = o;
  }
}


// Sliding audio window update, one pass: dst[b] = src[b][n:W] ++ chunk[b][0:n] (fp32, float4
// lanes; W, n multiples of 4).  Replaces two strided device copies per step.
__global__ __launch_bounds__(256) void window_shift_kernel(const float* __restrict__ src,
                                                           const float* __restrict__ chunk,
                                                           float* __restrict__ dst, int B, int W,
                                                           int n) {
  const int W4 = W >> 2, keep4 = (W - n) >> 2, n4 = n >> 2;
  const long total = (long)B * W4;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int b = (int)(idx / W4), i = (int)(idx - (long)b * W4);
    const f32x4 v = i < keep4 ? reinterpret_cast<const f32x4*>(src)[(long)b * W4 + i + n4]
                              : reinterpret_cast<const f32x4*>(chunk)[(long)b * n4 + (i - keep4)];
    reinterpret_cast<f32x4*>(dst)[idx] = v;
  }
}

}  // namespace aiko

extern "C" int aiko_logmel(const float* audio, int B, int N, const float* mel, int n_mels,
                           const int* mel_range, int n_fft, int hop, int F, float* logmel, int* gmax,
                           void* dst, int rows, int pad, int ld, hipStream_t stream) {
  if (n_fft > aiko::kMaxFFT || n_fft % 2 || n_mels > aiko::kMaxMels) return -1;
  hipMemsetAsync(gmax, 0x80, sizeof(int) * B, stream);  // 0x80808080: below every key
  dim3 grid((F + aiko::kFPB - 1) / aiko::kFPB, B);
  static const bool use_dft = [] { const char* e = getenv("AIKO_LOGMEL_DFT"); return e && *e == '1'; }();
  if (n_fft == 2 * aiko::kHalf && !use_dft && (aiko::kFPB - 1) * hop + n_fft <= aiko::kFPB * (aiko::kHalf + 1))
    aiko::logmel_fft400_kernel<<<grid, 256, 0, stream>>>(audio, N, mel, n_mels, mel_range, hop, F, logmel, gmax);
  else
    aiko::logmel_kernel<<<grid, 256, 0, stream>>>(audio, N, mel, n_mels, mel_range, n_fft, hop, F, logmel, gmax);
  const long total = (long)B * rows * n_mels;
  long g = (total + 255) / 256;
  if (g > 4096) g = 4096;
  const char* scalar = getenv("AIKO_LOGMEL_SCALAR");     // exactness tests: force the scalar path
  if (!(scalar && *scalar == '1') && n_mels % 8 == 0 && ld % 8 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(logmel) % 16 == 0 && total < (1L << 31)) {
    const long g8 = (total / 8 + 255) / 256;
    aiko::logmel_finalize8_kernel<<<(int)(g8 < 4096 ? g8 : 4096), 256, 0, stream>>>(
        logmel, gmax, static_cast<aiko::bf16_t*>(dst), B, F, n_mels, rows, pad, ld);
    return (int)hipGetLastError();
  }
  aiko::logmel_finalize_kernel<<<(int)g, 256, 0, stream>>>(logmel, gmax, static_cast<aiko::bf16_t*>(dst),
                                                          B, F, n_mels, rows, pad, ld);
  return (int)hipGetLastError();
}

extern "C" int aiko_window_shift(const float* src, const float* chunk, float* dst, int B, int W, int n,
                                 hipStream_t stream) {
  if (B <= 0 || n <= 0 || n > W || (W & 3) || (n & 3)) return -1;
  const long total = (long)B * (W >> 2);
  long g = (total + 255) / 256;
  if (g > 256 * 16) g = 256 * 16;
  aiko::window_shift_kernel<<<(int)g, 256, 0, stream>>>(src, chunk, dst, B, W, n);
  return (int)hipGetLastError();
}
