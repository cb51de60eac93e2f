// Antialiased resize (gfx950): uint8 [B, H, W, 3] frames -> uint8 [B, Ho, Wo, 3], separable and in
// fixed point, every byte what Pillow's Image.resize gives with the same filter.  The rule is stated
// in ops/scale.py: per axis a table of bounds (first, n) and a table of 22-bit coefficients k, made
// once on the host; a pass is out = clamp((2^21 + sum_x k[x] p[first + x]) >> 22, 0, 255) per
// channel.  The horizontal pass is rounded and clamped to bytes before the vertical pass reads it,
// so the two cannot be one sum.
//
// Three kernels, one per combination of passes:
//   scale_both_kernel  one workgroup per (frame, tile of a.tr output rows x a.tc output columns).
//                      The tile's source rows follow from the first and the last entry of the
//                      vertical bounds.  The horizontal pass of those rows, for the tile's columns,
//                      goes to LDS as bytes; after a barrier the vertical pass reads only LDS, four
//                      adjacent bytes per thread, and stores them packed.
//   scale_h_kernel     only the width changes: the horizontal pass straight to the output.
//   scale_v_kernel     only the height changes: the vertical pass straight from the frames, four
//                      adjacent bytes per thread (VEC: every row 4-byte aligned, dword loads).
// The coefficient tables are read from global memory (L2 keeps them): at high ratios they are too
// large for LDS.
//
// Sums are 32-bit: the plan maker guarantees 255 * sum|k| + 2^21 < 2^31 per output position, so no
// partial sum leaves int32.  They are added as unsigned words, where wrapping is defined, and read
// as int for the arithmetic shift.  The tables lie in HBM where the host cannot see them at launch
// time: every bound is clamped to the frame (and to the tile's LDS window) before it is used, so a
// table that does not follow the rule gives wrong bytes but never a read outside the frames.
//
// No float, no atomics, no scratch, every loop counted.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aiko_api.h"

namespace aiko {

constexpr int SC_THREADS = 256;
constexpr int SC_ROWS = 4;                            // source rows a horizontal-pass thread carries per column
constexpr int SC_MAX_COLS = 64;                       // output columns of a tile, at most
constexpr int SC_H_ROWS = SC_THREADS / SC_MAX_COLS * SC_ROWS;   // rows of a scale_h tile: one item per thread
constexpr int SC_V_BYTES = SC_THREADS * 4;            // output bytes of a scale_v workgroup
constexpr int SC_MAX_LDS = 160 * 1024;

struct ScaleArgs {
  const uint8_t* frames;
  uint8_t* out;
  const int2* hb;               // [Wo] (first, n); null without a horizontal pass
  const int* hk;                // [Wo, ksh]
  const int2* vb;               // [Ho]
  const int* vk;                // [Ho, ksv]
  int H, W, Ho, Wo, ksh, ksv;
  int tr, tc;                   // output rows and columns of a tile; tc a multiple of 4
  int win;                      // source rows of a tile, at most: the LDS holds win x tc x 3 bytes
};

__device__ __forceinline__ int sc_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ uint32_t sc_round(uint32_t acc) {
  return (uint32_t)sc_clamp((int)(acc + (1u << 21)) >> 22, 0, 255);
}

// the bounds of one output position, inside [0, size] and no longer than a table row
struct ScSpan {
  int first, n;
};

__device__ __forceinline__ ScSpan sc_span(int2 b, int size, int ksize) {
  ScSpan s;
  s.first = sc_clamp(b.x, 0, size);
  s.n = min(sc_clamp(b.y, 0, ksize), size - s.first);
  return s;
}

// One output column of SC_ROWS source rows: acc[i][c] += k[t] * row[i][(first + t) * 3 + c].  A
// coefficient is loaded once for its twelve bytes.
__device__ __forceinline__ void sc_hpass(const uint8_t* (&row)[SC_ROWS],const int* __restrict__ k, ScSpan s,
                                         uint32_t (&acc)[SC_ROWS][3]) {
#pragma unroll
  for (int i = 0; i < SC_ROWS; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[i][c] = 0;
  for (int t = 0; t < s.n; ++t) {
    const uint32_t kk = (uint32_t)k[t];
    const int off = (s.first + t) * 3;
#pragma unroll
    for (int i = 0; i < SC_ROWS; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[i][c] += kk * (uint32_t)row[i][off + c];
  }
}

// nb <= 4 bytes of v (byte i in bits 8i) to dst: one dword where it is whole and aligned
__device__ __forceinline__ void sc_store4(uint8_t* dst, uint32_t v, int nb) {
  if (nb == 4 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
    *reinterpret_cast<uint32_t*>(dst) = v;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nb) dst[i] = (uint8_t)(v >> (8 * i));
  }
}

// Grid (row tiles, column tiles, frames); dynamic LDS of a.win * a.tc * 3 bytes.
__global__ __launch_bounds__(SC_THREADS) void scale_both_kernel(const ScaleArgs a) {
  extern __shared__ uint32_t s_sc[];
  uint8_t* s_b = reinterpret_cast<uint8_t*>(s_sc);

  const int tid = threadIdx.x;
  const int y0 = blockIdx.x * a.tr, ny = min(a.tr, a.Ho - y0);
  const int x0 = blockIdx.y * a.tc, nc = min(a.tc, a.Wo - x0);
  const int pitch = a.tc * 3;                                          // bytes, a multiple of 4
  const long rowb = (long)a.W * 3;
  const uint8_t* frame = a.frames + (long)blockIdx.z * a.H * rowb;

  // the window: source rows [r0, r0 + wr)
  const ScSpan top = sc_span(a.vb[y0], a.H, a.ksv), bot = sc_span(a.vb[y0 + ny - 1], a.H, a.ksv);
  const int r0 = top.first;
  const int wr = sc_clamp(bot.first + bot.n - r0, 0, a.win);

  const int groups = (wr + SC_ROWS - 1) / SC_ROWS;
  for (int item = tid; item < groups * nc; item += SC_THREADS) {
    const int g = item / nc, x = item - g * nc;
    const ScSpan s = sc_span(a.hb[x0 + x], a.W, a.ksh);
    const uint8_t* row[SC_ROWS];
#pragma unroll
    for (int i = 0; i < SC_ROWS; ++i) row[i] = frame + (long)(r0 + min(g * SC_ROWS + i, wr - 1)) * rowb;
    uint32_t acc[SC_ROWS][3];
    sc_hpass(row, a.hk + (long)(x0 + x) * a.ksh, s, acc);
#pragma unroll
    for (int i = 0; i < SC_ROWS; ++i) {
      const int r = g * SC_ROWS + i;
      if (r < wr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s_b[r * pitch + x * 3 + c] = (uint8_t)sc_round(acc[i][c]);
      }
    }
  }
  __syncthreads();

  // a tile row's last dword may hold bytes no column wrote: they are summed and not stored
  const int ng = (nc * 3 + 3) / 4, pitchw = pitch / 4;
  uint8_t* out = a.out + ((long)blockIdx.z * a.Ho + y0) * a.Wo * 3 + (long)x0 * 3;
  for (int item = tid; item < ny * ng; item += SC_THREADS) {
    const int y = item / ng, g = item - y * ng;
    const ScSpan s = sc_span(a.vb[y0 + y], a.H, a.ksv);
    const int fv = sc_clamp(s.first - r0, 0, wr), nv = min(s.n, wr - fv);
    const int* __restrict__ k = a.vk + (long)(y0 + y) * a.ksv;
    const uint32_t* col = s_sc + fv * pitchw + g;
    uint32_t acc[4] = {0, 0, 0, 0};
    for (int t = 0; t < nv; ++t) {
      const uint32_t kk = (uint32_t)k[t], w = col[t * pitchw];
      acc[0] += kk * (w & 0xffu);
      acc[1] += kk * ((w >> 8) & 0xffu);
      acc[2] += kk * ((w >> 16) & 0xffu);
      acc[3] += kk * (w >> 24);
    }
    const uint32_t v = sc_round(acc[0]) | sc_round(acc[1]) << 8 | sc_round(acc[2]) << 16 | sc_round(acc[3]) << 24;
    sc_store4(out + (long)y * a.Wo * 3 + 4 * g, v, min(4, nc * 3 - 4 * g));
  }
}

// Grid (tiles of SC_H_ROWS rows, tiles of SC_MAX_COLS columns, frames): Ho = H.
__global__ __launch_bounds__(SC_THREADS) void scale_h_kernel(const ScaleArgs a) {
  const int y0 = blockIdx.x * SC_H_ROWS, nr = min(SC_H_ROWS, a.H - y0);
  const int x0 = blockIdx.y * SC_MAX_COLS, nc = min(SC_MAX_COLS, a.Wo - x0);
  const int item = threadIdx.x;
  const int g = item / nc, x = item - g * nc;
  if (g * SC_ROWS >= nr) return;
  const long rowb = (long)a.W * 3;
  const uint8_t* frame = a.frames + ((long)blockIdx.z * a.H + y0) * rowb;
  const ScSpan s = sc_span(a.hb[x0 + x], a.W, a.ksh);
  const uint8_t* row[SC_ROWS];
#pragma unroll
  for (int i = 0; i < SC_ROWS; ++i) row[i] = frame + (long)min(g * SC_ROWS + i, nr - 1) * rowb;
  uint32_t acc[SC_ROWS][3];
  sc_hpass(row, a.hk + (long)(x0 + x) * a.ksh, s, acc);
  uint8_t* out = a.out + (((long)blockIdx.z * a.H + y0) * a.Wo + x0 + x) * 3;
#pragma unroll
  for (int i = 0; i < SC_ROWS; ++i) {
    const int r = g * SC_ROWS + i;
    if (r < nr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) out[(long)r * a.Wo * 3 + c] = (uint8_t)sc_round(acc[i][c]);
    }
  }
}

// Grid (output rows, pieces of SC_V_BYTES bytes of a row, frames): Wo = W.
template <bool VEC>
__global__ __launch_bounds__(SC_THREADS) void scale_v_kernel(const ScaleArgs a) {
  const int y = blockIdx.x;
  const long rowb = (long)a.W * 3;
  const long j = ((long)blockIdx.y * SC_THREADS + threadIdx.x) * 4;
  if (j >= rowb) return;
  const int nb = (int)min(4L, rowb - j);
  const ScSpan s = sc_span(a.vb[y], a.H, a.ksv);
  const int* __restrict__ k = a.vk + (long)y * a.ksv;
  const uint8_t* src = a.frames + ((long)blockIdx.z * a.H + s.first) * rowb + j;
  uint32_t acc[4] = {0, 0, 0, 0};
  for (int t = 0; t < s.n; ++t) {
    const uint32_t kk = (uint32_t)k[t];
    const uint8_t* p = src + (long)t * rowb;
    uint32_t w = 0;
    if (VEC) {
      w = *reinterpret_cast<const uint32_t*>(p);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < nb) w |= (uint32_t)p[i] << (8 * i);
    }
    acc[0] += kk * (w & 0xffu);
    acc[1] += kk * ((w >> 8) & 0xffu);
    acc[2] += kk * ((w >> 16) & 0xffu);
    acc[3] += kk * (w >> 24);
  }
  const uint32_t v = sc_round(acc[0]) | sc_round(acc[1]) << 8 | sc_round(acc[2]) << 16 | sc_round(acc[3]) << 24;
  sc_store4(a.out + ((long)blockIdx.z * a.Ho + y) * rowb + j, v, nb);
}

}  // namespace aiko

// frames uint8 [B, H, W, 3] -> out uint8 [B, Ho, Wo, 3].  hb int32 [Wo, 2] (first, n) and hk int32
// [Wo, ksh]: the horizontal plan, both null when Wo = W and the pass is left out; vb [Ho, 2] and vk
// [Ho, ksv] likewise for the rows.  With both passes a workgroup makes tile_rows x tile_cols output
// pixels (tile_cols a multiple of 4, at most 64) from at most win_rows source rows, which it keeps
// in win_rows * tile_cols * 3 <= 160 KiB of LDS.  Returns -1 for a configuration the launch does
// not cover.
extern "C" int aiko_scale_frames(const void* frames, const int* hb, const int* hk, const int* vb, const int* vk,
                                 void* out, int B, int H, int W, int Ho, int Wo, int ksh, int ksv, int tile_rows,
                                 int tile_cols, int win_rows, hipStream_t stream) {
  const bool hp = hb != nullptr, vp = vb != nullptr;
  const int side = 1 << 24;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || H > side || W > side || Ho > side || Wo > side ||
      (!hp && !vp) || (hp && (!hk || ksh < 1)) || (vp && (!vk || ksv < 1)) || (!hp && Wo != W) || (!vp && Ho != H))
    return -1;
  aiko::ScaleArgs a;
  a.frames = static_cast<const uint8_t*>(frames);
  a.out = static_cast<uint8_t*>(out);
  a.hb = reinterpret_cast<const int2*>(hb);
  a.hk = hk;
  a.vb = reinterpret_cast<const int2*>(vb);
  a.vk = vk;
  a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.ksh = ksh; a.ksv = ksv;
  a.tr = tile_rows; a.tc = tile_cols; a.win = win_rows;
  if (hp && vp) {
    if (tile_rows < 1 || tile_cols < 4 || tile_cols > aiko::SC_MAX_COLS || tile_cols % 4 != 0 || win_rows < 1 ||
        win_rows > H || (long)win_rows * tile_cols * 3 > aiko::SC_MAX_LDS)
      return -1;
    const size_t lds = (size_t)win_rows * tile_cols * 3;
    const long cols = ((long)Wo + tile_cols - 1) / tile_cols;
    if (cols > 65535) return -1;
    if (lds > 64 * 1024) {                            // per device and function: set where it is needed
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&aiko::scale_both_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
    }
    const dim3 grid((unsigned)((Ho + tile_rows - 1) / tile_rows), (unsigned)cols, (unsigned)B);
    aiko::scale_both_kernel<<<grid, aiko::SC_THREADS, lds, stream>>>(a);
  } else if (hp) {
    const long cols = ((long)Wo + aiko::SC_MAX_COLS - 1) / aiko::SC_MAX_COLS;
    if (cols > 65535) return -1;
    const dim3 grid((unsigned)((H + aiko::SC_H_ROWS - 1) / aiko::SC_H_ROWS), (unsigned)cols, (unsigned)B);
    aiko::scale_h_kernel<<<grid, aiko::SC_THREADS, 0, stream>>>(a);
  } else {
    const long pieces = ((long)W * 3 + aiko::SC_V_BYTES - 1) / aiko::SC_V_BYTES;
    if (pieces > 65535) return -1;
    const dim3 grid((unsigned)Ho, (unsigned)pieces, (unsigned)B);
    const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(frames) % 4 == 0;
    if (vec)
      aiko::scale_v_kernel<true><<<grid, aiko::SC_THREADS, 0, stream>>>(a);
    else
      aiko::scale_v_kernel<false><<<grid, aiko::SC_THREADS, 0, stream>>>(a);
  }
  return (int)hipGetLastError();
}
