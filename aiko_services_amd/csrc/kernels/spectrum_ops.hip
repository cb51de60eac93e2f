// Spectrum analysis (gfx950): what is in this chunk, and how loud?  Mono fp32 chunks [B, n] (batch
// row b is stream b) -> the power of every frame (the spectrogram), the amplitude spectrum, its
// bands, its loudest points and, on request, the scatter graph of the points as an image.  Two or
// three launches per chunk, no host copy, no synchronisation, no state.  The rule is stated in
// ops/spectrum.py; ops/reference.py spectrum_ref gives the same bits.  Every fp32 and fp64 operation
// of the rule is rounded on its own: the arithmetic below stands under ``fp contract(off)`` and is
// written with the plain operators (roi_rect.h explains why __fmul_rn does not suffice).
//
//   * spectrum_frames_kernel: grid (F, B), one workgroup per frame.  The frame is read once (float4
//     when the rows and the hop allow it), cleaned, multiplied by the window and staged in LDS; a
//     thread keeps eight elements in registers through three radix-2 stages, so the 8 to 13 stages
//     cost three to five trips through LDS and as many barriers, and the bit reversal is part of
//     the first trip's addresses; the power of bins 0 .. n_fft/2 is stored coalesced.
//   * spectrum_reduce_kernel: one workgroup of 1024 threads per stream.  A thread owns bins tid, tid +
//     1024, ... and adds the frames' powers in order, eight loads under way at a time, coalesced across
//     the wave; the amplitudes go to LDS and HBM; one lane per band adds its bins from LDS; the kept
//     bins' 64-bit keys are gathered through an LDS counter and sorted in LDS by a bitonic network
//     whose comparators all point the same way, so that the slots past the kept count, up to the
//     next power of two, are never touched, and the first max_peaks keys are the peaks.
//   * spectrum_graph_kernel: grid (ceil(H / 16), B), one workgroup per strip of 16 image rows.  The
//     strip is cleared (the bottom axis included) 16 bytes a store, then, after a barrier each, the
//     left axis and the dots that touch the strip are stored over it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aiko_api.h"

namespace aiko {

constexpr int SP_THREADS = 256;
constexpr int SR_THREADS = 1024;                      // the reduce pass: a thread per bin up to n_fft 2048
constexpr int SP_MAX_F = 4096;                        // frames per call and stream
constexpr int SP_MAX_K = 4097;                        // bins at n_fft 8192
constexpr int SP_MAX_BANDS = 64;
constexpr int SP_MAX_PEAKS = 128;
constexpr int SG_ROWS = 16;                           // image rows per workgroup of the graph pass

struct SpectrumFrameArgs {
  const float* audio;           // [B, n]
  const float* window;          // [n_fft]
  const float2* twiddle;        // [n_fft / 2]: (cos, -sin)
  float* power;                 // [B, F, K]
  int n, F, hop;
};

// step 1 of the rule: NaN and +-inf read as 0, then the clamp
__device__ __forceinline__ float sp_sample(float x) {
  if (!(fabsf(x) <= 3.4028234663852886e38f)) return 0.f;      // NaN compares false, inf is larger
  return fminf(fmaxf(x, -32768.0f), 32767.0f);
}

// R consecutive radix-2 stages, the first of them stage s (h = 2^(s-1)), on the 2^R elements a thread holds:
// e[i] is element j + i * h of a block of 2^(s-1+R) elements, j < h.  At stage s + q element i is in the
// lower half of its block of 2^(s+q) iff bit q of i is clear, and its index there is j + h * (i mod 2^q).
// The arithmetic is that of the rule's stages, one rounding per operation.
template <int LOG2N, int R>
__device__ __forceinline__ void sp_stages(float2 (&e)[1 << R], int s, int j, const float2* __restrict__ twiddle) {
#pragma clang fp contract(off)
  const int h = 1 << (s - 1);
#pragma unroll
  for (int q = 0; q < R; ++q) {
#pragma unroll
    for (int i = 0; i < (1 << R); ++i) {
      if (i & (1 << q)) continue;
      const float2 t2 = twiddle[(j + h * (i & ((1 << q) - 1))) << (LOG2N - s - q)];
      const float c = t2.x, d = t2.y;
      const float2 p = e[i], b = e[i + (1 << q)];
      const float tr = b.x * c - b.y * d;
      const float ti = b.x * d + b.y * c;
      e[i] = make_float2(p.x + tr, p.y + ti);
      e[i + (1 << q)] = make_float2(p.x - tr, p.y - ti);
    }
  }
}

// One round in LDS: stages s .. s+R-1 of every group of 2^R elements, then a barrier.
template <int LOG2N, int R>
__device__ __forceinline__ void sp_round(float2* z, int s, int tid, const float2* __restrict__ twiddle) {
  constexpr int N = 1 << LOG2N;
  const int h = 1 << (s - 1);
  for (int g = tid; g < (N >> R); g += SP_THREADS) {  // at most N / 2048 groups of 8 per thread, at least one of 2
    const int j = g & (h - 1);
    const int base = ((g >> (s - 1)) << (s - 1 + R)) + j;
    float2 e[1 << R];
#pragma unroll
    for (int i = 0; i < (1 << R); ++i) e[i] = z[base + i * h];
    sp_stages<LOG2N, R>(e, s, j, twiddle);
#pragma unroll
    for (int i = 0; i < (1 << R); ++i) z[base + i * h] = e[i];
  }
  __syncthreads();
}

// Grid (F, B).  VEC: the frame starts 16-byte aligned and n % 4 == 0, so a float4 is inside the row
// or past it as a whole.  The windowed samples are staged in LDS in their own order (they share the
// first half of z's bytes); a thread then takes the eight that end up in z[8g .. 8g+7] after the
// bit reversal, v[bitrev(g) + (N/8) * bitrev3(i)], runs stages 1 to 3 on them in registers and stores
// them side by side.  Stages 4 .. log2 N follow three at a time, the remaining one or two last.
template <int LOG2N, bool VEC>
__global__ __launch_bounds__(SP_THREADS) void spectrum_frames_kernel(const SpectrumFrameArgs a) {
#pragma clang fp contract(off)
  constexpr int N = 1 << LOG2N, K = N / 2 + 1;
  constexpr int G = N / 8, PER = (G + SP_THREADS - 1) / SP_THREADS;      // groups of the first round, per thread
  __shared__ __attribute__((aligned(16))) float2 z[N];        // 64 KB at 8192
  float* v = reinterpret_cast<float*>(z);
  const int tid = threadIdx.x, f = blockIdx.x, b = blockIdx.y;
  const long start = (long)f * a.hop;                 // < n, or 0 when n < n_fft
  const float* x = a.audio + (long)b * a.n + start;
  const int left = (int)min((long)N, (long)a.n - start);      // samples of the frame inside the row

  if constexpr (VEC) {
    for (int q = tid; q < N / 4; q += SP_THREADS) {   // N / 1024 passes, one at N <= 1024
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      if (4 * q < left) s = reinterpret_cast<const float4*>(x)[q];
      const float4 w = reinterpret_cast<const float4*>(a.window)[q];
      reinterpret_cast<float4*>(v)[q] =
          make_float4(sp_sample(s.x) * w.x, sp_sample(s.y) * w.y, sp_sample(s.z) * w.z, sp_sample(s.w) * w.w);
    }
  } else {
    for (int i = tid; i < N; i += SP_THREADS) {       // N / 256 passes
      const float s = i < left ? x[i] : 0.f;
      v[i] = sp_sample(s) * a.window[i];
    }
  }
  __syncthreads();

  float in[PER][8];                                   // every group is read before z, which v is part of, is written
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int g = tid + u * SP_THREADS;
    if (g < G) {
      const int r = (int)(__brev((unsigned)g) >> (32 - (LOG2N - 3)));
#pragma unroll
      for (int i = 0; i < 8; ++i) in[u][i] = v[r + G * (((i & 1) << 2) | (i & 2) | (i >> 2))];
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int g = tid + u * SP_THREADS;
    if (g < G) {
      float2 e[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) e[i] = make_float2(in[u][i], 0.f);
      sp_stages<LOG2N, 3>(e, 1, 0, a.twiddle);
#pragma unroll
      for (int i = 0; i < 8; ++i) z[8 * g + i] = e[i];
    }
  }
  __syncthreads();

#pragma unroll
  for (int s = 4; s + 2 <= LOG2N; s += 3) sp_round<LOG2N, 3>(z, s, tid, a.twiddle);
  if constexpr (LOG2N % 3 == 1) sp_round<LOG2N, 1>(z, LOG2N, tid, a.twiddle);
  if constexpr (LOG2N % 3 == 2) sp_round<LOG2N, 2>(z, LOG2N - 1, tid, a.twiddle);

  float* out = a.power + ((long)b * a.F + f) * K;
  for (int k = tid; k < K; k += SP_THREADS) {
    const float2 c = z[k];
    out[k] = c.x * c.x + c.y * c.y;
  }
}

struct SpectrumReduceArgs {
  const float* power;           // [B, F, K]
  const int* band_start;        // [bands + 1]
  float* amplitudes;            // [B, K]
  float* band_amplitudes;       // [B, bands]
  int* peak_bins;               // [B, max_peaks]
  float* peak_amplitudes;       // [B, max_peaks]
  int* peak_counts;             // [B]
  int F, K, bands, max_peaks;
  float inv_F, lo, hi;
  int k_lo, k_hi, local;
};

// Grid B, one workgroup per stream.
__global__ __launch_bounds__(SR_THREADS) void spectrum_reduce_kernel(const SpectrumReduceArgs a) {
#pragma clang fp contract(off)
  __shared__ float s_a[SP_MAX_K];
  __shared__ unsigned long long s_key[SP_MAX_K];
  __shared__ int s_kept;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int K = a.K, F = a.F;                         // K <= SP_MAX_K, F <= SP_MAX_F: the host refuses the rest
  const float* __restrict__ p = a.power + (long)b * F * K;
  if (tid == 0) s_kept = 0;

  for (int k = tid; k < K; k += SR_THREADS) {         // at most 5 bins per thread
    const float* pk = p + k;
    float acc = pk[0];
    int f = 1;
    for (; f + 8 <= F; f += 8) {                      // eight loads under way, added in the frames' order
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = pk[(long)(f + u) * K];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = acc + t[u];
    }
    for (; f < F; ++f) acc = acc + pk[(long)f * K];
    const float amp = sqrtf(acc * a.inv_F);           // correctly rounded: hipcc's default for sqrtf
    s_a[k] = amp;
    a.amplitudes[(long)b * K + k] = amp;
  }
  __syncthreads();

  if (tid < a.bands) {                                // one lane per band; the table is held to 0 .. K
    const int k0 = min(max(a.band_start[tid], 0), K);
    const int k1 = min(max(a.band_start[tid + 1], k0), K);
    float sum = 0.f;
    for (int k = k0; k < k1; ++k) sum = sum + s_a[k];
    a.band_amplitudes[(long)b * a.bands + tid] = sum;
  }

  // The kept bins' keys, gathered at the front of s_key in whatever order the LDS counter hands out:
  // the keys are unique and the sort below orders them.  Amplitudes are non-negative and never NaN,
  // so their bits order them.
  for (int k = tid; k < K; k += SR_THREADS) {
    const float v = s_a[k];
    bool keep = v >= a.lo && v <= a.hi && k >= a.k_lo && k <= a.k_hi;
    if (a.local) keep = keep && (k == 0 || v > s_a[k - 1]) && (k == K - 1 || v >= s_a[k + 1]);
    if (keep) s_key[atomicAdd(&s_kept, 1)] = ((unsigned long long)__float_as_uint(v) << 32) | (0xFFFFFFFFu - (unsigned)k);
  }
  __syncthreads();
  const int M = s_kept;                               // <= K

  // Descending bitonic sort of P >= M slots, P a power of two.  Every comparator (i, j), i < j, puts
  // the larger key at i, so the slots M .. P-1, which stand for keys below all others, never move
  // and are never touched.
  int logP = 1;
  while ((1 << logP) < M) ++logP;                     // at most 13 rounds
  const int half = 1 << (logP - 1);
  for (int ks = 1; ks <= logP; ++ks) {
    const int kh = 1 << (ks - 1);                     // half a block of 2^ks
    for (int t = tid; t < half; t += SR_THREADS) {    // the flip: i against its mirror image in the block
      const int o = t & (kh - 1);
      const int base = (t >> (ks - 1)) << ks;
      const int i = base + o, j = base + 2 * kh - 1 - o;
      if (j < M) {
        const unsigned long long x = s_key[i], y = s_key[j];
        if (x < y) { s_key[i] = y; s_key[j] = x; }
      }
    }
    __syncthreads();
    for (int ds = ks - 1; ds >= 1; --ds) {            // then halving distances
      const int d = 1 << (ds - 1);
      for (int t = tid; t < half; t += SR_THREADS) {
        const int i = ((t >> (ds - 1)) << ds) + (t & (d - 1)), j = i + d;
        if (j < M) {
          const unsigned long long x = s_key[i], y = s_key[j];
          if (x < y) { s_key[i] = y; s_key[j] = x; }
        }
      }
      __syncthreads();
    }
  }

  const int count = min(M, a.max_peaks);
  if (tid < a.max_peaks) {                            // max_peaks <= 128 < SR_THREADS
    const unsigned long long key = tid < count ? s_key[tid] : 0ull;
    const long o = (long)b * a.max_peaks + tid;
    a.peak_bins[o] = tid < count ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
    a.peak_amplitudes[o] = tid < count ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
  }
  if (tid == 0) a.peak_counts[b] = count;
}

struct SpectrumGraphArgs {
  const int* peak_bins;         // [B, max_peaks]
  const float* peak_amplitudes; // [B, max_peaks]
  const int* peak_counts;       // [B]
  const int* bin_px;            // [K]
  uint8_t* image;               // [B, H, W, 3]
  int H, W, K, max_peaks;
  double y_max;
  int r, g, bl;
};

// four bytes of the cleared image from offset o on: 128 from offset ``last``, the start of row H-1, on
__device__ __forceinline__ unsigned sg_clear_word(int o, int last) {
  if (o + 3 < last) return 0u;
  if (o >= last) return 0x80808080u;
  return (o + 1 >= last ? 0x8000u : 0u) | (o + 2 >= last ? 0x800000u : 0u) | 0x80000000u;
}

// Grid (ceil(H / SG_ROWS), B).
__global__ __launch_bounds__(SP_THREADS) void spectrum_graph_kernel(const SpectrumGraphArgs a) {
#pragma clang fp contract(off)
  __shared__ int s_px[SP_MAX_PEAKS], s_py[SP_MAX_PEAKS];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int H = a.H, W = a.W;
  const int r0 = blockIdx.x * SG_ROWS, r1 = min(r0 + SG_ROWS, H);
  const int count = min(max(a.peak_counts[b], 0), a.max_peaks);
  if (tid < SP_MAX_PEAKS) {
    int px = -1, py = 0;
    if (tid < count) {
      const int bin = a.peak_bins[(long)b * a.max_peaks + tid];
      if (bin >= 0 && bin < a.K) {
        px = min(max(a.bin_px[bin], 0), W - 1);
        const double y = (1.0 - (double)a.peak_amplitudes[(long)b * a.max_peaks + tid] / a.y_max) * (double)(H - 1);
        py = (int)fmin(fmax(y, 0.0), (double)(H - 1));        // NaN cannot arise from the rule's peaks; fmax drops one
      }
    }
    s_px[tid] = px;
    s_py[tid] = py;
  }

  // The strip's bytes [o0, o1) of this image: 0, and 128 from the start of row H-1 on; single bytes up
  // to the first 16-byte boundary and after the last, 16 bytes a store in between.  No division: a
  // byte's value depends only on which side of ``last`` it is.
  uint8_t* img = a.image + (long)b * H * W * 3;
  const int o0 = r0 * W * 3, o1 = r1 * W * 3;         // H * W * 3 <= 3 * 2^24
  const int last = (H - 1) * W * 3;
  const int mis = (int)(reinterpret_cast<uintptr_t>(img + o0) & 15u);
  const int w0 = min(o0 + ((16 - mis) & 15), o1);
  const int quads = (o1 - w0) / 16;
  const int w1 = w0 + 16 * quads;
  if (tid < w0 - o0) img[o0 + tid] = o0 + tid >= last ? 128 : 0;
  if (tid < o1 - w1) img[w1 + tid] = w1 + tid >= last ? 128 : 0;
  for (int i = tid; i < quads; i += SP_THREADS) {     // at most 16 * 4096 * 3 / 16 / 256 = 48 passes
    const int o = w0 + 16 * i;
    *reinterpret_cast<uint4*>(img + o) = make_uint4(sg_clear_word(o, last), sg_clear_word(o + 4, last),
                                                    sg_clear_word(o + 8, last), sg_clear_word(o + 12, last));
  }
  __syncthreads();                                    // the strip is cleared before column 0 is drawn on it
  if (tid < 3 * (r1 - r0)) img[(r0 + tid / 3) * W * 3 + tid % 3] = 128;       // at most 48 bytes
  __syncthreads();                                    // ... and column 0 (and s_px, s_py) is written before a dot lands

  for (int t = tid; t < 9 * count; t += SP_THREADS) { // at most 5 passes
    const int i = t / 9, d = t - 9 * i;
    const int px = s_px[i];
    if (px < 0) continue;
    const int y = min(max(s_py[i] + d / 3 - 1, 0), H - 1), x = min(max(px + d % 3 - 1, 0), W - 1);
    if (y < r0 || y >= r1) continue;
    uint8_t* o = img + ((long)y * W + x) * 3;
    o[0] = (uint8_t)a.r; o[1] = (uint8_t)a.g; o[2] = (uint8_t)a.bl;
  }
}

}  // namespace aiko

namespace {

int log2_fft(int n_fft) {
  for (int l = 8; l <= 13; ++l)
    if (n_fft == 1 << l) return l;
  return 0;
}

template <int LOG2N>
void launch_frames(const aiko::SpectrumFrameArgs& c, bool vec, dim3 grid, hipStream_t stream) {
  if (vec)
    aiko::spectrum_frames_kernel<LOG2N, true><<<grid, aiko::SP_THREADS, 0, stream>>>(c);
  else
    aiko::spectrum_frames_kernel<LOG2N, false><<<grid, aiko::SP_THREADS, 0, stream>>>(c);
}

bool spectrum_shape(int B, long n, int F, int n_fft, int hop) {
  return log2_fft(n_fft) && B >= 1 && B <= 65535 && n >= 1 && n <= INT32_MAX && hop >= 1 && hop <= n_fft &&
         F == (n < n_fft ? 1 : 1 + (int)((n - n_fft) / hop)) && F <= aiko::SP_MAX_F;
}

}  // namespace

// The entry points return -1 for a configuration the launches do not cover.
// Steps 1 to 4, the frame pass: audio fp32 [B, n] -> power [B, F, K].  F is the caller's frame count of step 2.
extern "C" int aiko_spectrum_frames(const float* audio, const float* window, const float* twiddle, float* power, int B,
                                    long n, int F, int n_fft, int hop, hipStream_t stream) {
  if (!spectrum_shape(B, n, F, n_fft, hop)) return -1;
  aiko::SpectrumFrameArgs c;
  c.audio = audio; c.window = window; c.twiddle = reinterpret_cast<const float2*>(twiddle); c.power = power;
  c.n = (int)n; c.F = F; c.hop = hop;
  const bool vec = reinterpret_cast<uintptr_t>(audio) % 16 == 0 && n % 4 == 0 && hop % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(window) % 16 == 0;
  const dim3 grid((unsigned)F, (unsigned)B);
  switch (log2_fft(n_fft)) {
    case 8: launch_frames<8>(c, vec, grid, stream); break;
    case 9: launch_frames<9>(c, vec, grid, stream); break;
    case 10: launch_frames<10>(c, vec, grid, stream); break;
    case 11: launch_frames<11>(c, vec, grid, stream); break;
    case 12: launch_frames<12>(c, vec, grid, stream); break;
    default: launch_frames<13>(c, vec, grid, stream); break;
  }
  return (int)hipGetLastError();
}

// Steps 5 to 7, the reduce pass: power [B, F, K] -> amplitudes [B, K], band_amplitudes [B, bands], peak_bins /
// peak_amplitudes [B, max_peaks], peak_counts [B].
extern "C" int aiko_spectrum_reduce(const float* power, const int* band_start, float* amplitudes,
                                    float* band_amplitudes, int* peak_bins, float* peak_amplitudes, int* peak_counts,
                                    int B, int F, int n_fft, int bands, int max_peaks, float inv_F, float lo, float hi,
                                    int k_lo, int k_hi, int local, hipStream_t stream) {
  if (!log2_fft(n_fft) || B < 1 || B > 65535 || F < 1 || F > aiko::SP_MAX_F || bands < 1 ||
      bands > aiko::SP_MAX_BANDS || max_peaks < 1 || max_peaks > aiko::SP_MAX_PEAKS)
    return -1;
  aiko::SpectrumReduceArgs r;
  r.power = power; r.band_start = band_start; r.amplitudes = amplitudes; r.band_amplitudes = band_amplitudes;
  r.peak_bins = peak_bins; r.peak_amplitudes = peak_amplitudes; r.peak_counts = peak_counts;
  r.F = F; r.K = n_fft / 2 + 1; r.bands = bands; r.max_peaks = max_peaks;
  r.inv_F = inv_F; r.lo = lo; r.hi = hi; r.k_lo = k_lo; r.k_hi = k_hi; r.local = local ? 1 : 0;
  aiko::spectrum_reduce_kernel<<<dim3((unsigned)B), aiko::SR_THREADS, 0, stream>>>(r);
  return (int)hipGetLastError();
}

// One step, steps 1 to 7: both passes on ``stream``, nothing launched unless both are covered.
extern "C" int aiko_spectrum(const float* audio, const float* window, const float* twiddle, const int* band_start,
                             float* power, float* amplitudes, float* band_amplitudes, int* peak_bins,
                             float* peak_amplitudes, int* peak_counts, int B, long n, int F, int n_fft, int hop,
                             int bands, int max_peaks, float inv_F, float lo, float hi, int k_lo, int k_hi, int local,
                             hipStream_t stream) {
  if (!spectrum_shape(B, n, F, n_fft, hop) || bands < 1 || bands > aiko::SP_MAX_BANDS || max_peaks < 1 ||
      max_peaks > aiko::SP_MAX_PEAKS)
    return -1;
  const int rc = aiko_spectrum_frames(audio, window, twiddle, power, B, n, F, n_fft, hop, stream);
  return rc ? rc
            : aiko_spectrum_reduce(power, band_start, amplitudes, band_amplitudes, peak_bins, peak_amplitudes,
                                   peak_counts, B, F, n_fft, bands, max_peaks, inv_F, lo, hi, k_lo, k_hi, local, stream);
}

// Step 8: the peaks -> image uint8 [B, H, W, 3].
extern "C" int aiko_spectrum_graph(const int* peak_bins, const float* peak_amplitudes, const int* peak_counts,
                                   const int* bin_px, void* image, int B, int H, int W, int K, int max_peaks,
                                   double y_max, int r, int g, int b, hipStream_t stream) {
  if (B < 1 || B > 65535 || H < 16 || H > 4096 || W < 16 || W > 4096 || K < 1 || max_peaks < 1 ||
      max_peaks > aiko::SP_MAX_PEAKS || !(y_max > 0.0))
    return -1;
  aiko::SpectrumGraphArgs c;
  c.peak_bins = peak_bins; c.peak_amplitudes = peak_amplitudes; c.peak_counts = peak_counts; c.bin_px = bin_px;
  c.image = static_cast<uint8_t*>(image);
  c.H = H; c.W = W; c.K = K; c.max_peaks = max_peaks; c.y_max = y_max; c.r = r; c.g = g; c.bl = b;
  const dim3 grid((unsigned)((H + aiko::SG_ROWS - 1) / aiko::SG_ROWS), (unsigned)B);
  aiko::spectrum_graph_kernel<<<grid, aiko::SP_THREADS, 0, stream>>>(c);
  return (int)hipGetLastError();
}
