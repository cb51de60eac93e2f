// uint8 RGB -> raw YUV frames on the device (gfx950): the inverse of yuv_ops.hip.  The [B, H, W, 3]
// batches the pipeline ends in become what their consumers take: NV12 for a hardware encoder,
// planar I420 / I444 for a Y4M file, YUYV for a camera loop-back.  Frames are tightly packed, in
// the layouts of yuv_ops.hip:
//
//   nv12   Y plane H*W, then ch rows of cw interleaved (U, V) pairs      cw = (W+1)/2, ch = (H+1)/2
//   i420   Y plane, U plane ch*cw, V plane ch*cw
//   i444   Y, U, V planes of H*W each
//   yuyv   Y0 U Y1 V per pixel pair, W even
//
// Luma is per pixel.  A chroma sample is computed from the mean RGB of the in-frame pixels that
// share it (the 2x2 block for nv12 / i420, 2 or 1 pixels at an odd right or bottom edge; the
// horizontal pair for yuyv; the pixel itself for i444): an integer sum of bytes, converted to
// float and multiplied by 1/n, n in {1, 2, 4} — both exact, so the order of the sum cannot matter.
// The arithmetic is fp32 in a fixed order without FMA contraction, so each output byte equals
// ops/reference.py's rgb_to_yuv_ref bit for bit.
// Resources: no scratch, no LDS (12 KiB per workgroup in the vector kernels if built with
// AIKO_RGB_YUV_LDS_LOAD=1).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aiko_api.h"

// 0: each lane loads its own 48 RGB bytes per row (three uint4; across a wave 64 pieces 48 B apart,
// every line of the 3 KiB read in full by the three loads together).  1: a wave's row comes through
// LDS so that each load of a wave is 1 KiB contiguous, the mirror of yuv_ops.hip's store side.
// Measured at B = 192 of 480 x 640 (profiles/rgb_to_yuv.md): 0 is faster for nv12, i420 and yuyv
// and equal for i444 — strided loads do not cost what strided stores do — so 0 is what is built.
#ifndef AIKO_RGB_YUV_LDS_LOAD
#define AIKO_RGB_YUV_LDS_LOAD 0
#endif

namespace aiko {

constexpr int YUVO_THREADS = 256;
constexpr int YUVO_VPX = 16;                          // adjacent pixels of a thread per row, vector kernel
constexpr int YUVO_BPX = 2;                           // ... byte kernel
enum { YUVO_NV12 = 0, YUVO_I420 = 1, YUVO_I444 = 2, YUVO_YUYV = 3 };

struct RgbYuvArgs {
  const uint8_t* rgb;
  uint8_t* out;
  int H, W, cw, ch;
  int gpr;                      // threads per row: ceil(W / pixels per thread)
  int units;                    // threads per frame: gpr * rows (row pairs for the 4:2:0 formats)
  long frame_bytes;
  float yoff, yr, yg, yb, ur, ug, ub, vr, vg, vb;
  int half;                     // 0: rintf then clamp; 1: + 0.5f, clamp, truncate
};

// x rounded by the standard's rule and clamped: an integer in [0, 255], still as a float.
// HALF: x + 0.5, clamp, truncate (floor: the clamped value is not negative); else rint, clamp.
template <bool HALF>
__device__ __forceinline__ float yuvo_level(float x) {
  if (HALF) return floorf(__builtin_amdgcn_fmed3f(x + 0.5f, 0.0f, 255.0f));
  return __builtin_amdgcn_fmed3f(rintf(x), 0.0f, 255.0f);
}

// ((cr*r + cg*g) + cb*b) + off, rounded: the order of operations is the contract (see ops/yuv.py),
// no product is fused into the sum that uses it.
template <bool HALF>
__device__ __forceinline__ float yuvo_sample(float cr, float cg, float cb, float off, float r, float g, float b) {
#pragma clang fp contract(off)
  const float pr = cr * r, pg = cg * g, pb = cb * b;
  const float s = (pr + pg) + pb;
  return yuvo_level<HALF>(s + off);
}

// Byte k of a row of output bytes held as dwords <- level x (an exact integer: the conversion has
// nothing to round); k is a constant after unrolling.
__device__ __forceinline__ void yuvo_put(uint32_t* w, int k, float x) {
  w[k >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(x, k & 3, w[k >> 2]);
}

// Byte i of a little-endian word array; i is a constant after unrolling.
__device__ __forceinline__ uint32_t yuvo_byte(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// Grid (ceil(units / YUVO_THREADS), B).  Thread t of a frame owns PX adjacent pixels of row unit
// t / gpr — one row, or the two luma rows that share a chroma row for nv12 / i420, so that a 2x2
// block stays inside one thread — and consecutive threads read and write consecutive addresses,
// across row ends too.
// VEC: W % 16 == 0 and both tensors 16-byte aligned.  Every plane, row and frame offset is then a
// multiple of the load or store that uses it (the host wrapper checks this).  A thread's 48 RGB
// bytes per row are three uint4, loaded by the thread itself; with AIKO_RGB_YUV_LDS_LOAD lane L
// loads the uint4 at 16 (64 k + L), k = 0..2 — piece (64 k + L) % 3 of lane (64 k + L) / 3 —
// writes it to LDS at the same offset and reads back its own 48 bytes at 48 L.
// The stores are contiguous across lanes as they are: 16 luma bytes as one uint4, the chroma of 16
// pixels as 16 (nv12), 8 + 8 (i420) or 16 + 16 bytes (i444), 16 yuyv pixels as two uint4.
// !VEC: 2 pixels per thread and row, byte loads and stores: any width, any alignment.
template <int FMT, bool VEC, bool HALF>
__device__ __forceinline__ void rgb_to_yuv_body(const RgbYuvArgs& a, uint4* s_row) {
  constexpr int PX = VEC ? YUVO_VPX : YUVO_BPX;
  constexpr int ROWS = (FMT == YUVO_NV12 || FMT == YUVO_I420) ? 2 : 1;
  const int t = blockIdx.x * YUVO_THREADS + threadIdx.x;
  const bool live = t < a.units;
  if (!(VEC && AIKO_RGB_YUV_LDS_LOAD) && !live) return;   // the LDS variant has barriers ahead
  const int ru = t / a.gpr;
  const int x0 = (t - ru * a.gpr) * PX, y0 = ru * ROWS;
  const long W = a.W, HW = (long)a.H * a.W;
  const uint8_t* src = a.rgb + (long)blockIdx.y * HW * 3;
  uint8_t* dst = a.out + (long)blockIdx.y * a.frame_bytes;

  if constexpr (VEC) {
    uint32_t w[ROWS][12];                             // the thread's 16 pixels per row; zero past the frame
#if AIKO_RGB_YUV_LDS_LOAD
    const int lane = threadIdx.x & 63;
    uint4* s_wave = s_row + (threadIdx.x - lane) * 3;
    // the three pieces this lane loads: their owners' row units and columns (the same for both
    // rows of a 4:2:0 unit)
    uint4 q[ROWS][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int c = 64 * k + lane, j = c / 3;
      const int tj = t - lane + j;
      const int rj = tj / a.gpr;
      const long x3 = (long)(tj - rj * a.gpr) * (YUVO_VPX * 3) + (c - 3 * j) * 16;
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const int y = rj * ROWS + r;
        q[r][k] = make_uint4(0, 0, 0, 0);
        if (tj < a.units && y < a.H)                  // the owner is live and has this row
          q[r][k] = *reinterpret_cast<const uint4*>(src + (long)y * W * 3 + x3);
      }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      if (r > 0) __syncthreads();                     // the previous row has been read
#pragma unroll
      for (int k = 0; k < 3; ++k) s_wave[64 * k + lane] = q[r][k];
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint4 v = s_wave[3 * lane + k];
        w[r][4 * k] = v.x; w[r][4 * k + 1] = v.y; w[r][4 * k + 2] = v.z; w[r][4 * k + 3] = v.w;
      }
    }
#else
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (live && y0 + r < a.H) v = *reinterpret_cast<const uint4*>(src + ((long)(y0 + r) * W + x0) * 3 + 16 * k);
        w[r][4 * k] = v.x; w[r][4 * k + 1] = v.y; w[r][4 * k + 2] = v.z; w[r][4 * k + 3] = v.w;
      }
    }
#endif
    if (!live) return;                                // no barrier below
    const bool two = ROWS == 2 && y0 + 1 < a.H;       // odd H: the last chroma row serves one luma row

    if (FMT == YUVO_YUYV) {
      uint32_t o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int p = 0; p < YUVO_VPX / 2; ++p) {
        uint32_t s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = yuvo_byte(w[0], 6 * p + c) + yuvo_byte(w[0], 6 * p + 3 + c);
        const float rm = (float)s[0] * 0.5f, gm = (float)s[1] * 0.5f, bm = (float)s[2] * 0.5f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int b = 6 * p + 3 * i;
          yuvo_put(o, 4 * p + 2 * i, yuvo_sample<HALF>(a.yr, a.yg, a.yb, a.yoff, (float)yuvo_byte(w[0], b),
                                                       (float)yuvo_byte(w[0], b + 1), (float)yuvo_byte(w[0], b + 2)));
        }
        yuvo_put(o, 4 * p + 1, yuvo_sample<HALF>(a.ur, a.ug, a.ub, 128.0f, rm, gm, bm));
        yuvo_put(o, 4 * p + 3, yuvo_sample<HALF>(a.vr, a.vg, a.vb, 128.0f, rm, gm, bm));
      }
      uint4* d = reinterpret_cast<uint4*>(dst + ((long)y0 * W + x0) * 2);
      d[0] = make_uint4(o[0], o[1], o[2], o[3]);
      d[1] = make_uint4(o[4], o[5], o[6], o[7]);
    } else {
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        if (r > 0 && !two) break;
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < YUVO_VPX; ++i)
          yuvo_put(o, i, yuvo_sample<HALF>(a.yr, a.yg, a.yb, a.yoff, (float)yuvo_byte(w[r], 3 * i),
                                           (float)yuvo_byte(w[r], 3 * i + 1), (float)yuvo_byte(w[r], 3 * i + 2)));
        *reinterpret_cast<uint4*>(dst + (long)(y0 + r) * W + x0) = make_uint4(o[0], o[1], o[2], o[3]);
      }
      if (FMT == YUVO_I444) {
        uint32_t ou[4] = {0, 0, 0, 0}, ov[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < YUVO_VPX; ++i) {
          const float r = (float)yuvo_byte(w[0], 3 * i), g = (float)yuvo_byte(w[0], 3 * i + 1),
                      b = (float)yuvo_byte(w[0], 3 * i + 2);
          yuvo_put(ou, i, yuvo_sample<HALF>(a.ur, a.ug, a.ub, 128.0f, r, g, b));
          yuvo_put(ov, i, yuvo_sample<HALF>(a.vr, a.vg, a.vb, 128.0f, r, g, b));
        }
        const long off = (long)y0 * W + x0;
        *reinterpret_cast<uint4*>(dst + HW + off) = make_uint4(ou[0], ou[1], ou[2], ou[3]);
        *reinterpret_cast<uint4*>(dst + 2 * HW + off) = make_uint4(ov[0], ov[1], ov[2], ov[3]);
      } else {
        // nv12: bytes 2p, 2p + 1 of one uint4; i420: byte p of o[0..1] (U) and of o[2..3] (V)
        uint32_t o[4] = {0, 0, 0, 0};
        const float inv = two ? 0.25f : 0.5f;         // the missing row is zero in w[1]
#pragma unroll
        for (int p = 0; p < YUVO_VPX / 2; ++p) {
          uint32_t s[3];
#pragma unroll
          for (int c = 0; c < 3; ++c)
            s[c] = (yuvo_byte(w[0], 6 * p + c) + yuvo_byte(w[0], 6 * p + 3 + c)) +
                   (yuvo_byte(w[ROWS - 1], 6 * p + c) + yuvo_byte(w[ROWS - 1], 6 * p + 3 + c));
          const float rm = (float)s[0] * inv, gm = (float)s[1] * inv, bm = (float)s[2] * inv;
          const float u = yuvo_sample<HALF>(a.ur, a.ug, a.ub, 128.0f, rm, gm, bm);
          const float v = yuvo_sample<HALF>(a.vr, a.vg, a.vb, 128.0f, rm, gm, bm);
          yuvo_put(o, FMT == YUVO_NV12 ? 2 * p : p, u);
          yuvo_put(o, FMT == YUVO_NV12 ? 2 * p + 1 : 8 + p, v);
        }
        if (FMT == YUVO_NV12) {
          *reinterpret_cast<uint4*>(dst + HW + (long)ru * (2 * a.cw) + x0) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
          const long plane = (long)a.ch * a.cw, off = (long)ru * a.cw + (x0 >> 1);
          *reinterpret_cast<uint2*>(dst + HW + off) = make_uint2(o[0], o[1]);
          *reinterpret_cast<uint2*>(dst + HW + plane + off) = make_uint2(o[2], o[3]);
        }
      }
    }
  } else {
    uint32_t s[3] = {0, 0, 0};                        // the chroma sample's byte sums and pixel count
    int n = 0;
    float lum[ROWS][PX];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int y = y0 + r;
#pragma unroll
      for (int i = 0; i < PX; ++i) {
        const int x = x0 + i;
        lum[r][i] = 0.0f;
        if (y >= a.H || x >= a.W) continue;
        const uint8_t* p = src + (y * W + x) * 3;
        const uint32_t R = p[0], G = p[1], B = p[2];
        lum[r][i] = yuvo_sample<HALF>(a.yr, a.yg, a.yb, a.yoff, (float)R, (float)G, (float)B);
        if (FMT == YUVO_I444) {
          uint8_t* q = dst + y * W + x;
          q[0] = (uint8_t)lum[r][i];
          q[HW] = (uint8_t)yuvo_sample<HALF>(a.ur, a.ug, a.ub, 128.0f, (float)R, (float)G, (float)B);
          q[2 * HW] = (uint8_t)yuvo_sample<HALF>(a.vr, a.vg, a.vb, 128.0f, (float)R, (float)G, (float)B);
        } else {
          if (FMT != YUVO_YUYV) dst[y * W + x] = (uint8_t)lum[r][i];
          s[0] += R; s[1] += G; s[2] += B;
          ++n;
        }
      }
    }
    if (FMT != YUVO_I444) {                           // n >= 1: the thread's first pixel is in the frame
      const float inv = n == 4 ? 0.25f : n == 2 ? 0.5f : 1.0f;
      const float rm = (float)s[0] * inv, gm = (float)s[1] * inv, bm = (float)s[2] * inv;
      const uint8_t u = (uint8_t)yuvo_sample<HALF>(a.ur, a.ug, a.ub, 128.0f, rm, gm, bm);
      const uint8_t v = (uint8_t)yuvo_sample<HALF>(a.vr, a.vg, a.vb, 128.0f, rm, gm, bm);
      if (FMT == YUVO_NV12) {
        uint8_t* c = dst + HW + ((long)ru * a.cw + (x0 >> 1)) * 2;
        c[0] = u; c[1] = v;
      } else if (FMT == YUVO_I420) {
        uint8_t* c = dst + HW + (long)ru * a.cw + (x0 >> 1);
        c[0] = u; c[(long)a.ch * a.cw] = v;
      } else {
        uint8_t* c = dst + (y0 * W + x0) * 2;         // W is even: the pair is complete
        c[0] = (uint8_t)lum[0][0]; c[1] = u; c[2] = (uint8_t)lum[0][1]; c[3] = v;
      }
    }
  }
}

// The rounding mode is uniform: one branch per thread, straight-line code behind it.
template <int FMT, bool VEC>
__global__ __launch_bounds__(YUVO_THREADS) void rgb_to_yuv_kernel(const RgbYuvArgs a) {
  // with AIKO_RGB_YUV_LDS_LOAD: 12 KiB, 64 x 48 B per wave, the vector kernel's rows
  __shared__ uint4 s_row[(VEC && AIKO_RGB_YUV_LDS_LOAD) ? YUVO_THREADS * 3 : 1];
  if (a.half)
    rgb_to_yuv_body<FMT, VEC, true>(a, s_row);
  else
    rgb_to_yuv_body<FMT, VEC, false>(a, s_row);
}

template <int FMT>
static int rgb_yuv_launch(const RgbYuvArgs& a, bool vec, dim3 grid, hipStream_t stream) {
  if (vec)
    rgb_to_yuv_kernel<FMT, true><<<grid, YUVO_THREADS, 0, stream>>>(a);
  else
    rgb_to_yuv_kernel<FMT, false><<<grid, YUVO_THREADS, 0, stream>>>(a);
  return (int)hipGetLastError();
}

}  // namespace aiko

// rgb uint8 [B, H, W, 3] -> out uint8 [B, frame_bytes].  coef = yoff, yr, yg, yb, ur, ug, ub, vr,
// vg, vb; half selects the rounding.  The vector kernel runs iff W % 16 == 0 and rgb and out are
// 16-byte aligned.  Returns -1 for a configuration the launch does not cover.
extern "C" int aiko_rgb_to_yuv_u8(const void* rgb, void* out, int B, int H, int W, int fmt, const float* coef,
                                  int half, hipStream_t stream) {
  using namespace aiko;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 32768 || W > 32768 || fmt < YUVO_NV12 || fmt > YUVO_YUYV ||
      (half != 0 && half != 1) || (fmt == YUVO_YUYV && W % 2 != 0))
    return -1;
  RgbYuvArgs a;
  a.rgb = static_cast<const uint8_t*>(rgb);
  a.out = static_cast<uint8_t*>(out);
  a.H = H; a.W = W; a.cw = (W + 1) / 2; a.ch = (H + 1) / 2;
  const long HW = (long)H * W, cplane = (long)a.ch * a.cw;
  a.frame_bytes = fmt == YUVO_I444 ? 3 * HW : fmt == YUVO_YUYV ? 2 * HW : HW + 2 * cplane;
  a.yoff = coef[0]; a.yr = coef[1]; a.yg = coef[2]; a.yb = coef[3];
  a.ur = coef[4]; a.ug = coef[5]; a.ub = coef[6];
  a.vr = coef[7]; a.vg = coef[8]; a.vb = coef[9];
  a.half = half;
  bool vec = W % YUVO_VPX == 0 && reinterpret_cast<uintptr_t>(rgb) % 16 == 0 &&
             reinterpret_cast<uintptr_t>(out) % 16 == 0;
  if (vec) {
    // the offsets the vector kernel adds to the aligned bases, each against the load or store that
    // uses it: RGB rows and frames (uint4 loads), output frames, luma rows and planes (uint4 stores)
    const long row = fmt == YUVO_YUYV ? 2 * (long)W : W;
    vec = (W * 3L) % 16 == 0 && (HW * 3) % 16 == 0 && a.frame_bytes % 16 == 0 && row % 16 == 0 && HW % 16 == 0;
    if (fmt == YUVO_NV12) vec = vec && (2 * a.cw) % 16 == 0;            // chroma rows, uint4 stores
    if (fmt == YUVO_I420) vec = vec && a.cw % 8 == 0 && cplane % 8 == 0; // chroma rows and planes, uint2 stores
  }
  const int rows = (fmt == YUVO_NV12 || fmt == YUVO_I420) ? a.ch : H;
  const int px = vec ? YUVO_VPX : YUVO_BPX;
  a.gpr = (W + px - 1) / px;
  a.units = rows * a.gpr;                             // <= 32768 * 16384
  const dim3 grid((unsigned)((a.units + YUVO_THREADS - 1) / YUVO_THREADS), (unsigned)B);
  switch (fmt) {
    case YUVO_NV12: return rgb_yuv_launch<YUVO_NV12>(a, vec, grid, stream);
    case YUVO_I420: return rgb_yuv_launch<YUVO_I420>(a, vec, grid, stream);
    case YUVO_I444: return rgb_yuv_launch<YUVO_I444>(a, vec, grid, stream);
    default: return rgb_yuv_launch<YUVO_YUYV>(a, vec, grid, stream);
  }
}
