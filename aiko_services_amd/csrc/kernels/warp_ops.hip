// Projective warp of uint8 frames selected by quads (gfx950): ``quads`` [B, Kq, 4, 2] + ``count`` [B]
// (the marker detector's corners and counts, marker_ops.hip, or one fixed quad per camera) select K
// quadrilaterals per frame, each rectified to Ho x Wo uint8 without the quads or the count ever
// visiting the host.  The rule is stated in ops/warp.py and equals ops/reference.py warp_quads_ref
// (numpy float64) bit for bit: exact int64 coefficients, fp64 per pixel with one rounding per
// operation, integer bilinear sampling in 1/256 of a pixel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aiko_api.h"

namespace aiko {

constexpr int WARP_BAND = 32;       // patch rows per workgroup: 8 per wave, the columns' u computed once for them

// The three bytes of the pixel at byte offset ``off`` of ``frames`` in the low 24 bits: one
// unaligned dword load.  The pixel that ends the tensor is read one byte early and shifted, so no
// byte past ``total`` (the tensor's size, >= 4) is touched.
__device__ __forceinline__ uint32_t warp_load_rgb(const uint8_t* __restrict__ frames, long off, long total) {
  const int back = off + 4 > total ? 1 : 0;
  uint32_t v;
  __builtin_memcpy(&v, frames + off - back, 4);
  return v >> (8 * back);
}

// Steps 3 (from px, py on) and 4 of the rule: the pixel at the doubled continuous position (px, py) of
// the frame at ``base``, RGB in the low 24 bits.  tx, ty are clamped into [0, (W-1)*256] x [0, (H-1)*256]
// before they become integers and the second taps are clamped again, so every tap lies in the frame
// whatever px, py are (infinities included; they are never NaN).
__device__ __forceinline__ uint32_t warp_sample(const uint8_t* __restrict__ frames, long base, long total, int W,
                                                int H, double px, double py, double xmax, double ymax) {
#pragma clang fp contract(off)
  const double tx = fmin(fmax(px * 128.0 - 127.5, 0.0), xmax);
  const double ty = fmin(fmax(py * 128.0 - 127.5, 0.0), ymax);
  const int Px = (int)tx, Py = (int)ty;                       // tx, ty >= 0: the truncation is the floor
  const int xi = Px >> 8, yi = Py >> 8;
  const uint32_t fx = Px & 255, fy = Py & 255;
  const int xj = min(xi + 1, W - 1), yj = min(yi + 1, H - 1);
  const uint32_t p00 = warp_load_rgb(frames, base + (long)(yi * W + xi) * 3, total);
  const uint32_t p01 = warp_load_rgb(frames, base + (long)(yi * W + xj) * 3, total);
  const uint32_t p10 = warp_load_rgb(frames, base + (long)(yj * W + xi) * 3, total);
  const uint32_t p11 = warp_load_rgb(frames, base + (long)(yj * W + xj) * 3, total);
  const uint32_t w00 = (256u - fx) * (256u - fy), w01 = fx * (256u - fy), w10 = (256u - fx) * fy, w11 = fx * fy;
  uint32_t v = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {                               // the weights sum to 65536: below 2^32
    const uint32_t s = w00 * ((p00 >> (8 * c)) & 0xffu) + w01 * ((p01 >> (8 * c)) & 0xffu) +
                       w10 * ((p10 >> (8 * c)) & 0xffu) + w11 * ((p11 >> (8 * c)) & 0xffu) + 32768u;
    v |= (s >> 16) << (8 * c);
  }
  return v;
}

// patches[b*K + i] <- quad i of frame b rectified to Ho x Wo; valid[b*K + i] <- 1 iff the slot is used
// (i < min(max(count[b], 0), K), the eight coordinates in -4096..8191, den != 0); an unused slot gets
// zeros and its quad is not read past the count.
// Grid (bands of WARP_BAND patch rows, B*K): a workgroup stays inside one slot, so the nine coefficients
// and the decision are computed once per workgroup from eight scalar-loaded integers.  The four waves
// take the band's rows in turn (a row is wave-uniform: v and its three products are per row), a lane
// owns four adjacent pixels of a row (12 bytes, three dword stores) and keeps their u products over
// the rows; rows wider than 256 pixels are walked in chunks of 64 lanes.  fp64 with the plain operators
// under ``fp contract(off)`` (roi_rect.h says why); the divisions are the compiler's IEEE ones.
__global__ __launch_bounds__(256) void quad_warp_u8_kernel(
    const uint8_t* __restrict__ frames, const int* __restrict__ quads, const int* __restrict__ count,
    uint8_t* __restrict__ patches, int* __restrict__ valid, int H, int W, int Kq, int K, int Ho, int Wo, int m,
    int o, long total) {
#pragma clang fp contract(off)
  const int slot = blockIdx.y;
  const int b = slot / K, i = slot - b * K;
  const int Wq = Wo >> 2;                                     // lanes per patch row
  const int row0 = blockIdx.x * WARP_BAND, rows = min(WARP_BAND, Ho - row0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t* out = reinterpret_cast<uint32_t*>(patches + (long)slot * Ho * Wo * 3) + (long)row0 * Wq * 3;

  bool used = i < min(max(count[b], 0), K);                   // workgroup-uniform from here on
  long G = 0, Hh = 0, den = 0, A = 0, Bx = 0, Cx = 0, D = 0, E = 0, Cy = 0;
  if (used) {
    const int* q = quads + ((long)b * Kq + i) * 8;
    int lo = q[0], hi = q[0];
#pragma unroll
    for (int n = 1; n < 8; ++n) { lo = min(lo, q[n]); hi = max(hi, q[n]); }
    used = lo >= -4096 && hi <= 8191;
    if (used) {
      const long X0 = 2 * q[0] + o, Y0 = 2 * q[1] + o, X1 = 2 * q[2] + o, Y1 = 2 * q[3] + o;
      const long X2 = 2 * q[4] + o, Y2 = 2 * q[5] + o, X3 = 2 * q[6] + o, Y3 = 2 * q[7] + o;
      const long dx1 = X1 - X2, dx2 = X3 - X2, sx = X0 - X1 + X2 - X3;
      const long dy1 = Y1 - Y2, dy2 = Y3 - Y2, sy = Y0 - Y1 + Y2 - Y3;
      den = dx1 * dy2 - dy1 * dx2;
      G = sx * dy2 - sy * dx2;
      Hh = dx1 * sy - dy1 * sx;
      A = den * (X1 - X0) + G * X1; Bx = den * (X3 - X0) + Hh * X3; Cx = den * X0;
      D = den * (Y1 - Y0) + G * Y1; E = den * (Y3 - Y0) + Hh * Y3; Cy = den * Y0;
      if (den < 0) { G = -G; Hh = -Hh; den = -den; A = -A; Bx = -Bx; Cx = -Cx; D = -D; E = -E; Cy = -Cy; }
      used = den != 0;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) valid[slot] = used ? 1 : 0;

  if (!used) {                                                // the band is rows * Wq * 3 contiguous dwords
    const int n = rows * Wq * 3;
    if ((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (n & 3) == 0) {
      uint4* out4 = reinterpret_cast<uint4*>(out);
      for (int t = threadIdx.x; t < (n >> 2); t += 256) out4[t] = make_uint4(0u, 0u, 0u, 0u);
    } else {
      for (int t = threadIdx.x; t < rows * Wq; t += 256) {
        out[t * 3] = 0u; out[t * 3 + 1] = 0u; out[t * 3 + 2] = 0u;
      }
    }
    return;
  }

  // every coefficient is below 2^53 in magnitude: the conversions are exact
  const double dG = (double)G, dH = (double)Hh, dden = (double)den, dA = (double)A, dB = (double)Bx, dCx = (double)Cx;
  const double dD = (double)D, dE = (double)E, dCy = (double)Cy;
  const double ud = (double)(16 * Wo), vd = (double)(16 * Ho);
  const double xmax = (double)((W - 1) * 256), ymax = (double)((H - 1) * 256);
  const long base = (long)b * H * W * 3;
  const int a = 8 + m;

  for (int q0 = 0; q0 < Wq; q0 += 64) {
    const int q = q0 + lane;
    const bool on = q < Wq;
    double Gu[4], Au[4], Du[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = q * 4 + e;
      const double u = (double)((2 * j + 1) * a - m * Wo) / ud;
      Gu[e] = dG * u; Au[e] = dA * u; Du[e] = dD * u;
    }
    for (int r = wave; r < rows; r += 4) {
      const int y = row0 + r;
      const double v = (double)((2 * y + 1) * a - m * Ho) / vd;
      const double Hv = dH * v, Bv = dB * v, Ev = dE * v;
      if (!on) continue;
      uint32_t px[4];                                         // 4 patch pixels, RGB in the low 24 bits
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double w = (Gu[e] + Hv) + dden;
        const double X = (Au[e] + Bv) + dCx;
        const double Y = (Du[e] + Ev) + dCy;
        const bool front = w > 0.0;
        const double ws = front ? w : 1.0;                    // behind the horizon: sampled like any pixel, then zero
        const uint32_t p = warp_sample(frames, base, total, W, H, X / ws, Y / ws, xmax, ymax);
        px[e] = front ? p : 0u;
      }
      uint32_t* dst = out + ((long)r * Wq + q) * 3;
      dst[0] = px[0] | (px[1] << 24);
      dst[1] = (px[1] >> 8) | (px[2] << 16);
      dst[2] = (px[2] >> 16) | (px[3] << 8);
    }
  }
}

}  // namespace aiko

// frames uint8 [B, H, W, 3] (>= 4 bytes, H, W <= 4096), quads int32 [B, Kq, 4, 2], count int32 [B] ->
// patches uint8 [B*K, Ho, Wo, 3] (4-byte aligned), valid int32 [B*K]; margin 0..64 sixteenths of the
// side, origin 1 (coordinates are pixel centres) or 0 (pixel edges)
extern "C" int aiko_quad_warp_u8(const void* frames, const int* quads, const int* count, void* patches, int* valid,
                                 int B, int H, int W, int Kq, int K, int Ho, int Wo, int margin, int origin,
                                 hipStream_t stream) {
  if (B < 1 || H < 1 || W < 1 || H > 4096 || W > 4096 || K < 1 || K > Kq || Ho < 1 || Ho > 4096 || Wo < 4 ||
      Wo > 4096 || Wo % 4 || margin < 0 || margin > 64 || (origin != 0 && origin != 1))
    return -1;
  const long total = (long)B * H * W * 3, slots = (long)B * K;
  if (total < 4 || slots > 65535) return -1;
  if (reinterpret_cast<uintptr_t>(patches) % 4 || reinterpret_cast<uintptr_t>(valid) % 4) return -1;
  const dim3 grid((unsigned)((Ho + aiko::WARP_BAND - 1) / aiko::WARP_BAND), (unsigned)slots);
  aiko::quad_warp_u8_kernel<<<grid, 256, 0, stream>>>(static_cast<const uint8_t*>(frames), quads, count,
                                                      static_cast<uint8_t*>(patches), valid, H, W, Kq, K, Ho, Wo,
                                                      margin, origin, total);
  return (int)hipGetLastError();
}
