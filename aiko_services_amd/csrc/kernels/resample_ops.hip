// Raw PCM -> mono fp32 at another sample rate on the device (gfx950): downmix and band-limited
// polyphase resampling of what a sound card or a WAV file delivers (interleaved int16 or fp32 at
// 44.1 / 48 kHz, often stereo) into the [B, n] fp32 chunks the speech path reads.
//
//   mono, int16:  float(int32 sum of the C samples) * scale          scale = float(1 / (32768 C))
//   mono, fp32:   ((x0 + x1) + ...) * scale                          scale = float(1 / C)
//   s[b]        = hist[b] ++ mono[b]                                 T-1 + n_in samples
//   out[b][j]   = acc after  acc = 0; for k = 0..T-1: acc = acc + filt[p][k] * s[b][i0 + k]
//                 with i0 = (j M) / L, p = (j M) % L
//   hist_out[b] = s[b][n_in : n_in + T-1]
//
// All fp32, in this order, no product fused into the sum that uses it: the output equals
// ops/reference.py's resample_ref bit for bit.  The order within an output is fixed; the
// parallelism is across outputs.
//
// Grid (tiles + 1, B).  Workgroup x < tiles owns RS_TILE consecutive outputs of stream y: it copies
// the L*T taps into LDS, downmixes the span of s its outputs read into LDS once (from hist where
// the span starts inside it), then every thread runs RS_CHAINS independent outputs, RS_THREADS
// apart, so that a wave's LDS reads are M/L samples apart (conflict-free for odd M, L = 1).
// Workgroup x == tiles writes hist_out of its stream: the tiles' spans end up to ceil(M/L) - 1
// samples short of s's end, and for n_in < T-1 hist_out is mostly old history, so no tile owns it.
// VEC: C <= 2, pcm 16-byte aligned and a row a multiple of 16 bytes: a thread loads 16 bytes,
// 8 / 4 int16 or 4 / 2 fp32 frames, and keeps the frames inside the span.  !VEC: any C <= 8, any
// alignment, one frame per thread and step.
// Resources: no scratch; dynamic LDS 4 * (L*T + span) bytes, at most 160 KiB (the host checks).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aiko_api.h"

namespace aiko {

constexpr int RS_THREADS = 256;
#ifndef AIKO_RS_CHAINS
#define AIKO_RS_CHAINS 4                              // 2 and 8 were timed: profiles/audio_resample.md
#endif
constexpr int RS_CHAINS = AIKO_RS_CHAINS;             // outputs of a thread
#ifndef AIKO_RS_TAP_LOADS
#define AIKO_RS_TAP_LOADS 4                           // 1 was timed: profiles/audio_resample.md
#endif
constexpr int RS_TAP_LOADS = AIKO_RS_TAP_LOADS;       // 16-byte tap loads a thread keeps in flight
constexpr int RS_TILE = RS_THREADS * RS_CHAINS;       // outputs of a workgroup
constexpr int RS_MAX_TAPS = 16384;                    // L*T: 64 KiB of taps
constexpr int RS_MAX_LDS = 160 * 1024;

struct ResampleArgs {
  const void* pcm;
  const float* hist;
  const float* filt;
  float* out;
  float* hist_out;
  int n_in, n_out, C, L, M, T;
  int tiles;                    // ceil(n_out / RS_TILE)
  int filt_vec;                 // filt 16-byte aligned and L*T % 4 == 0
  float scale;
};

// One frame of C interleaved samples -> mono.  The order of operations is the contract.
__device__ __forceinline__ float rs_mono(const int16_t* f, int C, float scale) {
#pragma clang fp contract(off)
  int sum = f[0];
  for (int c = 1; c < C; ++c) sum += f[c];
  return (float)sum * scale;
}

__device__ __forceinline__ float rs_mono(const float* f, int C, float scale) {
#pragma clang fp contract(off)
  float sum = f[0];
  for (int c = 1; c < C; ++c) sum = sum + f[c];
  return sum * scale;
}

__device__ __forceinline__ int rs_lo(uint32_t w) { return (int)(int16_t)(w & 0xffffu); }
__device__ __forceinline__ int rs_hi(uint32_t w) { return (int)(int16_t)(w >> 16); }

// The frames of one aligned 16-byte vector, C in {1, 2}: put(i, mono of the vector's frame i).
template <typename Put>
__device__ __forceinline__ void rs_mono_vec(const int16_t*, uint4 q, int C, float scale, Put put) {
#pragma clang fp contract(off)
  if (C == 1) {
    put(0, (float)rs_lo(q.x) * scale); put(1, (float)rs_hi(q.x) * scale);
    put(2, (float)rs_lo(q.y) * scale); put(3, (float)rs_hi(q.y) * scale);
    put(4, (float)rs_lo(q.z) * scale); put(5, (float)rs_hi(q.z) * scale);
    put(6, (float)rs_lo(q.w) * scale); put(7, (float)rs_hi(q.w) * scale);
  } else {
    put(0, (float)(rs_lo(q.x) + rs_hi(q.x)) * scale);
    put(1, (float)(rs_lo(q.y) + rs_hi(q.y)) * scale);
    put(2, (float)(rs_lo(q.z) + rs_hi(q.z)) * scale);
    put(3, (float)(rs_lo(q.w) + rs_hi(q.w)) * scale);
  }
}

template <typename Put>
__device__ __forceinline__ void rs_mono_vec(const float*, uint4 q, int C, float scale, Put put) {
#pragma clang fp contract(off)
  const float x0 = __uint_as_float(q.x), x1 = __uint_as_float(q.y), x2 = __uint_as_float(q.z),
              x3 = __uint_as_float(q.w);
  if (C == 1) {
    put(0, x0 * scale); put(1, x1 * scale); put(2, x2 * scale); put(3, x3 * scale);
  } else {
    put(0, (x0 + x1) * scale);
    put(1, (x2 + x3) * scale);
  }
}

template <typename S, bool VEC>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const ResampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const int tid = threadIdx.x;
  const int T = a.T, L = a.L, M = a.M, C = a.C;
  const long b = blockIdx.y;
  const S* pcm = static_cast<const S*>(a.pcm) + b * a.n_in * C;
  const float* hist = a.hist + b * (T - 1);

  if ((int)blockIdx.x == a.tiles) {                   // hist_out[b] = s[b][n_in : n_in + T-1]
    float* ho = a.hist_out + b * (T - 1);
    for (int i = tid; i < T - 1; i += RS_THREADS) {
      const long idx = (long)a.n_in + i;              // <= n_in + T-2, the last element of s
      ho[i] = idx < T - 1 ? hist[idx] : rs_mono(pcm + (idx - (T - 1)) * C, C, a.scale);
    }
    return;
  }

  float* s_taps = rs_lds;
  float* s_span = rs_lds + L * T;
  const int taps = L * T;
  if (a.filt_vec) {
    const float4* f4 = reinterpret_cast<const float4*>(a.filt);
    float4* t4 = reinterpret_cast<float4*>(s_taps);
    // several loads in flight per thread: with one load and one wait per step the 57.6 KB table
    // of 44.1 kHz is fourteen L2 round trips in a row
    const int n4 = taps / 4;
    int i = tid;
    for (; i + (RS_TAP_LOADS - 1) * RS_THREADS < n4; i += RS_TAP_LOADS * RS_THREADS) {
      float4 v[RS_TAP_LOADS];
#pragma unroll
      for (int u = 0; u < RS_TAP_LOADS; ++u) v[u] = f4[i + u * RS_THREADS];
#pragma unroll
      for (int u = 0; u < RS_TAP_LOADS; ++u) t4[i + u * RS_THREADS] = v[u];
    }
    for (; i < n4; i += RS_THREADS) t4[i] = f4[i];
  } else {
    for (int i = tid; i < taps; i += RS_THREADS) s_taps[i] = a.filt[i];
  }

  // this tile's outputs [j0, j0 + n) read s[lo, hi)
  const long j0 = (long)blockIdx.x * RS_TILE;
  const int n = (int)(a.n_out - j0 < RS_TILE ? a.n_out - j0 : RS_TILE);
  const long lo = j0 * M / L;
  const long hi = (j0 + n - 1) * M / L + T;           // <= n_in + T-1
  for (long i = lo + tid; i < hi && i < T - 1; i += RS_THREADS) s_span[i - lo] = hist[i];
  const long f_lo = lo > T - 1 ? lo - (T - 1) : 0;    // frames [f_lo, f_hi) of pcm
  const long f_hi = hi - (T - 1);                     // <= n_in
  const long shift = (T - 1) - lo;                    // frame f is s[f + T-1], at s_span[f + shift]
  if (VEC) {
    constexpr int SLOTS = 16 / (int)sizeof(S);        // samples of a vector
    const int F = SLOTS / C;                          // frames of a vector: n_in % F == 0
    const uint4* rows = reinterpret_cast<const uint4*>(pcm);
    for (long v = f_lo / F + tid; v * F < f_hi; v += RS_THREADS) {
      const long f0 = v * F;
      rs_mono_vec(pcm, rows[v], C, a.scale, [&](int i, float m) {
        const long f = f0 + i;
        if (f >= f_lo && f < f_hi) s_span[f + shift] = m;   // the frames of the vector inside the span
      });
    }
  } else {
    for (long f = f_lo + tid; f < f_hi; f += RS_THREADS) s_span[f + shift] = rs_mono(pcm + f * C, C, a.scale);
  }
  __syncthreads();

  int so[RS_CHAINS], to[RS_CHAINS];                   // offsets of a chain's samples and taps in LDS
  long jc[RS_CHAINS];
#pragma unroll
  for (int c = 0; c < RS_CHAINS; ++c) {
    long j = j0 + tid + c * RS_THREADS;
    jc[c] = j;
    if (j >= j0 + n) j = j0 + n - 1;                  // a dead chain repeats the tile's last output
    const long jm = j * M;
    const long i0 = L == 1 ? jm : jm / L;
    so[c] = (int)(i0 - lo);
    to[c] = (int)(jm - i0 * L) * T;
  }
  float acc[RS_CHAINS];
#pragma unroll
  for (int c = 0; c < RS_CHAINS; ++c) acc[c] = 0.0f;
  {
#pragma clang fp contract(off)
    if (L == 1) {                                     // one row: the tap is the same for all chains
#pragma unroll 4
      for (int k = 0; k < T; ++k) {
        const float w = s_taps[k];
#pragma unroll
        for (int c = 0; c < RS_CHAINS; ++c) {
          const float prod = w * s_span[so[c] + k];
          acc[c] = acc[c] + prod;
        }
      }
    } else {
#pragma unroll 2
      for (int k = 0; k < T; ++k) {
#pragma unroll
        for (int c = 0; c < RS_CHAINS; ++c) {
          const float prod = s_taps[to[c] + k] * s_span[so[c] + k];
          acc[c] = acc[c] + prod;
        }
      }
    }
  }
  float* out = a.out + b * a.n_out;
#pragma unroll
  for (int c = 0; c < RS_CHAINS; ++c)
    if (jc[c] < j0 + n) out[jc[c]] = acc[c];
}

template <typename S>
static int resample_launch(const ResampleArgs& a, bool vec, dim3 grid, size_t lds, hipStream_t stream) {
  const void* fn = vec ? reinterpret_cast<const void*>(&resample_kernel<S, true>)
                       : reinterpret_cast<const void*>(&resample_kernel<S, false>);
  if (lds > 64 * 1024) {                              // per device and function: set where it is needed
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  if (vec)
    resample_kernel<S, true><<<grid, RS_THREADS, lds, stream>>>(a);
  else
    resample_kernel<S, false><<<grid, RS_THREADS, lds, stream>>>(a);
  return (int)hipGetLastError();
}

}  // namespace aiko

// pcm [B, n_in, C] int16 (is_f32 = 0) or fp32, hist [B, T-1], filt [L, T] -> out [B, n_out],
// hist_out [B, T-1], n_out = n_in L / M.  The vector kernel runs iff C <= 2, pcm is 16-byte aligned
// and a row of pcm is a multiple of 16 bytes.  Returns -1 for a configuration the launch does not
// cover.
extern "C" int aiko_resample(const void* pcm, int is_f32, const float* hist, const float* filt, float* out,
                             float* hist_out, int B, long n_in, int C, int L, int M, int T, hipStream_t stream) {
  using namespace aiko;
  if (B < 1 || B > 65535 || n_in < 1 || C < 1 || C > 8 || L < 1 || M < 1 || T < 1 || (long)L * T > RS_MAX_TAPS ||
      n_in * L % M != 0 || n_in + T > INT32_MAX || n_in * C > INT32_MAX)
    return -1;
  const long n_out = n_in * L / M;
  if (n_out < 1 || n_out > INT32_MAX - RS_TILE) return -1;
  const long span = ((long)(RS_TILE - 1) * M + L - 1) / L + T;     // the most samples of s a tile reads
  const long lds = 4 * ((long)L * T + span);
  if (lds > RS_MAX_LDS) return -1;
  ResampleArgs a;
  a.pcm = pcm; a.hist = hist; a.filt = filt; a.out = out; a.hist_out = hist_out;
  a.n_in = (int)n_in; a.n_out = (int)n_out; a.C = C; a.L = L; a.M = M; a.T = T;
  a.tiles = (int)((n_out + RS_TILE - 1) / RS_TILE);
  a.filt_vec = reinterpret_cast<uintptr_t>(filt) % 16 == 0 && (L * T) % 4 == 0;
  const long esize = is_f32 ? 4 : 2;
  a.scale = is_f32 ? (float)(1.0 / C) : (float)(1.0 / (32768.0 * C));
  const bool vec = C <= 2 && reinterpret_cast<uintptr_t>(pcm) % 16 == 0 && (n_in * C * esize) % 16 == 0;
  const dim3 grid((unsigned)(a.tiles + 1), (unsigned)B);
  return is_f32 ? resample_launch<float>(a, vec, grid, (size_t)lds, stream)
                : resample_launch<int16_t>(a, vec, grid, (size_t)lds, stream);
}
