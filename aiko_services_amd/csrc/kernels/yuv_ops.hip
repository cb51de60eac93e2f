// Raw YUV frames -> uint8 RGB on the device (gfx950): what a hardware decoder (NV12), a camera
// (YUYV) or a Y4M file (I420 / I444) delivers, converted into the [B, H, W, 3] batches every
// other kernel of the project reads.  Frames are tightly packed: no row pitch, no padded planes.
//
//   nv12   Y plane H*W, then ch rows of cw interleaved (U, V) pairs      cw = (W+1)/2, ch = (H+1)/2
//   i420   Y plane, U plane ch*cw, V plane ch*cw
//   i444   Y, U, V planes of H*W each
//   yuyv   Y0 U Y1 V per pixel pair, W even
//
// Chroma is replicated, never interpolated: pixel (y, x) uses sample (y/2, x/2), (y, x/2) for yuyv.
// The arithmetic is one function for all formats, fp32 in a fixed order without FMA contraction,
// so each output byte equals the host converters' and ops/reference.py's bit for bit.
// Resources: no scratch; the vector kernels use 12 KiB of LDS per workgroup to make their stores
// contiguous, the byte kernels none.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aiko_api.h"

namespace aiko {

constexpr int YUV_THREADS = 256;
constexpr int YUV_VPX = 16;                           // adjacent pixels of a thread per row, vector kernel
constexpr int YUV_BPX = 2;                            // ... byte kernel
enum { YUV_NV12 = 0, YUV_I420 = 1, YUV_I444 = 2, YUV_YUYV = 3 };

struct YuvArgs {
  const uint8_t* raw;
  uint8_t* out;
  int H, W, cw, ch;
  int gpr;                      // threads per row: ceil(W / pixels per thread)
  int units;                    // threads per frame: gpr * rows (row pairs for the 4:2:0 formats)
  long frame_bytes;
  float yoff, ygain, rv, gu, gv, bu;
  int half;                     // 0: rintf then clamp; 1: + 0.5f, clamp, truncate
};

// x rounded by the standard's rule and clamped: an integer in [0, 255], still as a float.
// HALF: x + 0.5, clamp, truncate (floor: the clamped value is not negative); else rint, clamp.
template <bool HALF>
__device__ __forceinline__ float yuv_level(float x) {
  if (HALF) return floorf(__builtin_amdgcn_fmed3f(x + 0.5f, 0.0f, 255.0f));
  return __builtin_amdgcn_fmed3f(rintf(x), 0.0f, 255.0f);
}

// One pixel -> its three levels.  The order of operations is the contract (see ops/yuv.py): no
// product is fused into the sum that uses it.
template <bool HALF>
__device__ __forceinline__ void yuv_pixel(uint32_t Y, uint32_t U, uint32_t V, const YuvArgs& a, float& r, float& g,
                                          float& b) {
#pragma clang fp contract(off)
  const float c = ((float)Y - a.yoff) * a.ygain;
  const float u = (float)U - 128.0f, v = (float)V - 128.0f;
  r = yuv_level<HALF>(c + a.rv * v);
  g = yuv_level<HALF>((c - a.gu * u) - a.gv * v);
  b = yuv_level<HALF>(c + a.bu * u);
}

// Byte k of a row of packed RGB pixels held as dwords <- level x (an exact integer: the
// conversion has nothing to round); k is a constant after unrolling.
__device__ __forceinline__ void put_byte(uint32_t* w, int k, float x) {
  w[k >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(x, k & 3, w[k >> 2]);
}

// Byte i of a little-endian word array; i is a constant after unrolling.
__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// Grid (ceil(units / YUV_THREADS), B).  Thread t of a frame owns PX adjacent pixels of row unit
// t / gpr — one row, or the two luma rows that share a chroma row for nv12 / i420 — so consecutive
// threads read and write consecutive addresses, across row ends too.
// VEC: W % 16 == 0 and both tensors 16-byte aligned.  Every plane and row offset is then a
// multiple of the load that reads it (the host wrapper checks this): 16 luma bytes as one uint4,
// the chroma of 16 pixels as 16 (nv12, i444: U and V each) or 8 + 8 bytes (i420), 16 yuyv pixels
// as two uint4.  A thread's 48 output bytes per row are three uint4, but stored from the owning
// lanes a wave's store would touch 64 pieces of 16 B, 48 B apart; three such stores write every
// line three times over and cost 41 us where contiguous ones cost 26 (profiles/yuv_to_rgb.md).
// So a wave's row goes through LDS: lane L writes its 48 bytes at 48 L and reads the uint4 at
// 16 (64 k + L), k = 0..2 — piece (64 k + L) % 3 of lane (64 k + L) / 3 — and stores that, so that
// every store of a wave covers 1 KiB without gaps (two runs where the wave spans a row end).
// !VEC: 2 pixels per thread and row, byte loads and stores: any width, any alignment.
template <int FMT, bool VEC, bool HALF>
__device__ __forceinline__ void yuv_to_rgb_body(const YuvArgs& a, uint4* s_row) {
  constexpr int PX = VEC ? YUV_VPX : YUV_BPX;
  constexpr int ROWS = (FMT == YUV_NV12 || FMT == YUV_I420) ? 2 : 1;
  const int t = blockIdx.x * YUV_THREADS + threadIdx.x;
  const bool live = t < a.units;
  if (!VEC && !live) return;                          // the vector kernel has barriers ahead
  const int ru = t / a.gpr;
  const int x0 = (t - ru * a.gpr) * PX, y0 = ru * ROWS;
  const long W = a.W, HW = (long)a.H * a.W;
  const uint8_t* src = a.raw + (long)blockIdx.y * a.frame_bytes;
  uint8_t* dst = a.out + (long)blockIdx.y * HW * 3;

  if constexpr (VEC) {
    const int lane = threadIdx.x & 63;
    uint4* s_wave = s_row + (threadIdx.x - lane) * 3;
    // the three pieces this lane stores: their owners' row units and columns (the same for both
    // rows of a 4:2:0 unit)
    int p_ru[3], p_x3[3];                             // row unit (-1: no owner), byte column in the row
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int c = 64 * k + lane, j = c / 3;
      const int tj = t - lane + j;
      const int rj = tj / a.gpr;
      p_ru[k] = tj < a.units ? rj : -1;
      p_x3[k] = (tj - rj * a.gpr) * (YUV_VPX * 3) + (c - 3 * j) * 16;
    }
    uint32_t cw[8] = {0, 0, 0, 0, 0, 0, 0, 0};        // chroma words (yuyv: the 16 pixels themselves)
    if (!live) {
    } else if (FMT == YUV_NV12) {
      const uint4 q = *reinterpret_cast<const uint4*>(src + HW + (long)ru * (2 * a.cw) + x0);
      cw[0] = q.x; cw[1] = q.y; cw[2] = q.z; cw[3] = q.w;
    } else if (FMT == YUV_I420) {
      const long plane = (long)a.ch * a.cw, off = (long)ru * a.cw + (x0 >> 1);
      const uint2 qu = *reinterpret_cast<const uint2*>(src + HW + off);
      const uint2 qv = *reinterpret_cast<const uint2*>(src + HW + plane + off);
      cw[0] = qu.x; cw[1] = qu.y; cw[2] = qv.x; cw[3] = qv.y;
    } else if (FMT == YUV_I444) {
      const long off = (long)y0 * W + x0;
      const uint4 qu = *reinterpret_cast<const uint4*>(src + HW + off);
      const uint4 qv = *reinterpret_cast<const uint4*>(src + 2 * HW + off);
      cw[0] = qu.x; cw[1] = qu.y; cw[2] = qu.z; cw[3] = qu.w;
      cw[4] = qv.x; cw[5] = qv.y; cw[6] = qv.z; cw[7] = qv.w;
    } else {
      const uint4* q = reinterpret_cast<const uint4*>(src + ((long)y0 * W + x0) * 2);
      const uint4 q0 = q[0], q1 = q[1];
      cw[0] = q0.x; cw[1] = q0.y; cw[2] = q0.z; cw[3] = q0.w;
      cw[4] = q1.x; cw[5] = q1.y; cw[6] = q1.z; cw[7] = q1.w;
    }
    uint32_t yw[ROWS][4];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      yw[r][0] = yw[r][1] = yw[r][2] = yw[r][3] = 0;
      if (FMT != YUV_YUYV && live && y0 + r < a.H) {
        const uint4 q = *reinterpret_cast<const uint4*>(src + (long)(y0 + r) * W + x0);
        yw[r][0] = q.x; yw[r][1] = q.y; yw[r][2] = q.z; yw[r][3] = q.w;
      }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      if (r > 0) __syncthreads();                     // the previous row has been read
      if (live && y0 + r < a.H) {                     // odd H: the last chroma row serves one luma row
        uint32_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < YUV_VPX; ++i) {
          uint32_t Y, U, V;
          if (FMT == YUV_NV12) {
            Y = byte_of(yw[r], i); U = byte_of(cw, i & ~1); V = byte_of(cw, i | 1);
          } else if (FMT == YUV_I420) {
            Y = byte_of(yw[r], i); U = byte_of(cw, i >> 1); V = byte_of(cw + 2, i >> 1);
          } else if (FMT == YUV_I444) {
            Y = byte_of(yw[r], i); U = byte_of(cw, i); V = byte_of(cw + 4, i);
          } else {
            Y = byte_of(cw, 2 * i); U = byte_of(cw, 4 * (i >> 1) + 1); V = byte_of(cw, 4 * (i >> 1) + 3);
          }
          float R, G, B;
          yuv_pixel<HALF>(Y, U, V, a, R, G, B);
          put_byte(o, 3 * i, R);
          put_byte(o, 3 * i + 1, G);
          put_byte(o, 3 * i + 2, B);
        }
        s_wave[3 * lane] = make_uint4(o[0], o[1], o[2], o[3]);
        s_wave[3 * lane + 1] = make_uint4(o[4], o[5], o[6], o[7]);
        s_wave[3 * lane + 2] = make_uint4(o[8], o[9], o[10], o[11]);
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int y = p_ru[k] * ROWS + r;
        if (p_ru[k] >= 0 && y < a.H)                  // the owner was live and wrote this row
          *reinterpret_cast<uint4*>(dst + (long)y * W * 3 + p_x3[k]) = s_wave[64 * k + lane];
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int y = y0 + r;
      if (y >= a.H) break;
#pragma unroll
      for (int i = 0; i < PX; ++i) {
        const int x = x0 + i;
        if (x >= a.W) break;
        uint32_t Y, U, V;
        if (FMT == YUV_NV12) {
          const uint8_t* c = src + HW + ((long)ru * a.cw + (x >> 1)) * 2;
          Y = src[y * W + x]; U = c[0]; V = c[1];
        } else if (FMT == YUV_I420) {
          const uint8_t* c = src + HW + (long)ru * a.cw + (x >> 1);
          Y = src[y * W + x]; U = c[0]; V = c[(long)a.ch * a.cw];
        } else if (FMT == YUV_I444) {
          const uint8_t* c = src + y * W + x;
          Y = c[0]; U = c[HW]; V = c[2 * HW];
        } else {
          const uint8_t* c = src + (y * W + (x & ~1)) * 2;   // W is even: the pair is complete
          Y = c[2 * (x & 1)]; U = c[1]; V = c[3];
        }
        float R, G, B;
        yuv_pixel<HALF>(Y, U, V, a, R, G, B);
        uint8_t* q = dst + (y * W + x) * 3;
        q[0] = (uint8_t)R;
        q[1] = (uint8_t)G;
        q[2] = (uint8_t)B;
      }
    }
  }
}

// The rounding mode is uniform: one branch per thread, straight-line code behind it.
template <int FMT, bool VEC>
__global__ __launch_bounds__(YUV_THREADS) void yuv_to_rgb_kernel(const YuvArgs a) {
  __shared__ uint4 s_row[VEC ? YUV_THREADS * 3 : 1];  // 12 KiB, 64 x 48 B per wave: the vector kernel's rows
  if (a.half)
    yuv_to_rgb_body<FMT, VEC, true>(a, s_row);
  else
    yuv_to_rgb_body<FMT, VEC, false>(a, s_row);
}

template <int FMT>
static int yuv_launch(const YuvArgs& a, bool vec, dim3 grid, hipStream_t stream) {
  if (vec)
    yuv_to_rgb_kernel<FMT, true><<<grid, YUV_THREADS, 0, stream>>>(a);
  else
    yuv_to_rgb_kernel<FMT, false><<<grid, YUV_THREADS, 0, stream>>>(a);
  return (int)hipGetLastError();
}

}  // namespace aiko

// raw uint8 [B, frame_bytes] -> out uint8 [B, H, W, 3].  coef = yoff, ygain, rv, gu, gv, bu; half
// selects the rounding.  The vector kernel runs iff W % 16 == 0 and raw and out are 16-byte
// aligned.  Returns -1 for a configuration the launch does not cover.
extern "C" int aiko_yuv_to_rgb_u8(const void* raw, void* out, int B, int H, int W, int fmt, const float* coef,
                                  int half, hipStream_t stream) {
  using namespace aiko;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 32768 || W > 32768 || fmt < YUV_NV12 || fmt > YUV_YUYV ||
      (half != 0 && half != 1) || (fmt == YUV_YUYV && W % 2 != 0))
    return -1;
  YuvArgs a;
  a.raw = static_cast<const uint8_t*>(raw);
  a.out = static_cast<uint8_t*>(out);
  a.H = H; a.W = W; a.cw = (W + 1) / 2; a.ch = (H + 1) / 2;
  const long HW = (long)H * W, cplane = (long)a.ch * a.cw;
  a.frame_bytes = fmt == YUV_I444 ? 3 * HW : fmt == YUV_YUYV ? 2 * HW : HW + 2 * cplane;
  a.yoff = coef[0]; a.ygain = coef[1]; a.rv = coef[2]; a.gu = coef[3]; a.gv = coef[4]; a.bu = coef[5];
  a.half = half;
  bool vec = W % YUV_VPX == 0 && reinterpret_cast<uintptr_t>(raw) % 16 == 0 &&
             reinterpret_cast<uintptr_t>(out) % 16 == 0;
  if (vec) {
    // the offsets the vector kernel adds to the aligned bases, each against the load that uses it
    const long row = fmt == YUV_YUYV ? 2 * (long)W : W;
    vec = a.frame_bytes % 16 == 0 && row % 16 == 0 && HW % 16 == 0 && (W * 3L) % 16 == 0;
    if (fmt == YUV_NV12) vec = vec && (2 * a.cw) % 16 == 0;
    if (fmt == YUV_I420) vec = vec && a.cw % 8 == 0 && cplane % 8 == 0;
  }
  const int rows = (fmt == YUV_NV12 || fmt == YUV_I420) ? a.ch : H;
  const int px = vec ? YUV_VPX : YUV_BPX;
  a.gpr = (W + px - 1) / px;
  a.units = rows * a.gpr;                             // <= 32768 * 16384
  const dim3 grid((unsigned)((a.units + YUV_THREADS - 1) / YUV_THREADS), (unsigned)B);
  switch (fmt) {
    case YUV_NV12: return yuv_launch<YUV_NV12>(a, vec, grid, stream);
    case YUV_I420: return yuv_launch<YUV_I420>(a, vec, grid, stream);
    case YUV_I444: return yuv_launch<YUV_I444>(a, vec, grid, stream);
    default: return yuv_launch<YUV_YUYV>(a, vec, grid, stream);
  }
}
