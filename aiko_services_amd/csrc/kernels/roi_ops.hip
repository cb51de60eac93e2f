// ROI crop for detect-then-classify cascades (gfx950): the fixed-size NMS output of the detector
// (``det`` [B, max_det, 6] + ``count`` [B], detect_ops.hip) selects K sub-images per frame, each
// resized to Ho x Wo uint8 — the input of ResNet50.logits — without the rows or the count ever
// visiting the host, so the cascade stays a chain of graph-replayable launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "roi_rect.h"
#include "aiko_api.h"

namespace aiko {

// The three bytes of the pixel at byte offset ``off`` of ``frames`` in the low 24 bits: one
// unaligned dword load.  The pixel that ends the tensor is read one byte early and shifted, so no
// byte past ``total`` (the tensor's size, >= 4) is touched.
__device__ __forceinline__ uint32_t load_rgb(const uint8_t* __restrict__ frames, long off, long total) {
  const int back = off + 4 > total ? 1 : 0;
  uint32_t v;
  __builtin_memcpy(&v, frames + off - back, 4);
  return v >> (8 * back);
}

__device__ __forceinline__ float chan(uint32_t v, int c) { return (float)((v >> (8 * c)) & 0xffu); }

// crops[b*K + k] <- bilinear resize (half-pixel centres, source coordinate clamped at 0, taps
// clamped to the rect: the sampling of resize_u8_kernel on the sub-image) of the rect of
// det[b, k]; rois[b*K + k] <- the rect.  Slot (b, k) is valid iff k < min(count[b], K) and its
// four coordinates are finite; an invalid slot gets zeros in both and det[b, k] is not read.
// Grid (pixel blocks, B*K): a workgroup stays inside one slot, so validity, rect and scales are
// wave-uniform.  One thread makes 4 adjacent output pixels (12 bytes, three dword stores).
__global__ __launch_bounds__(256) void roi_crop_u8_kernel(
    const uint8_t* __restrict__ frames, const float* __restrict__ det, const int* __restrict__ count,
    uint8_t* __restrict__ crops, int* __restrict__ rois, int H, int W, int max_det, int K, int Ho,
    int Wo, float margin, long total) {
  const int slot = blockIdx.y;
  const int b = slot / K, k = slot - b * K;
  const int Wq = Wo >> 2;                                   // threads per output row
  const int g = blockIdx.x * 256 + threadIdx.x;
  const bool active = g < Ho * Wq;
  const int yo = g / Wq, xq = g - yo * Wq;
  uint32_t* out = reinterpret_cast<uint32_t*>(crops + ((long)slot * Ho * Wo) * 3) + (long)g * 3;

  bool valid = k < min(max(count[b], 0), K);                // wave-uniform from here on
  RoiRect r{0, 0, 0, 0};
  if (valid) {
    const float* row = det + ((long)b * max_det + k) * 6;
    const float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
    valid = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
    if (valid) r = roi_rect(x1, y1, x2, y2, margin, H, W);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *reinterpret_cast<int4*>(rois + (long)slot * 4) = make_int4(r.x0, r.y0, r.x1, r.y1);
  if (!active) return;
  if (!valid) {
    out[0] = 0u; out[1] = 0u; out[2] = 0u;
    return;
  }

  const int Hr = r.y1 - r.y0, Wr = r.x1 - r.x0;
  const float sy_scale = (float)Hr / Ho, sx_scale = (float)Wr / Wo;
  const float sy = fmaxf((yo + 0.5f) * sy_scale - 0.5f, 0.f);
  const int y0 = min((int)sy, Hr - 1), y1 = min(y0 + 1, Hr - 1);
  const float fy = sy - y0;
  const long row0 = (((long)b * H + r.y0 + y0) * W + r.x0) * 3;
  const long row1 = (((long)b * H + r.y0 + y1) * W + r.x0) * 3;

  uint32_t px[4];                                           // 4 output pixels, RGB in the low 24 bits
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int xo = xq * 4 + i;
    const float sx = fmaxf((xo + 0.5f) * sx_scale - 0.5f, 0.f);
    const int x0 = min((int)sx, Wr - 1), x1 = min(x0 + 1, Wr - 1);
    const float fx = sx - x0;
    const uint32_t p00 = load_rgb(frames, row0 + x0 * 3, total);
    const uint32_t p01 = load_rgb(frames, row0 + x1 * 3, total);
    const uint32_t p10 = load_rgb(frames, row1 + x0 * 3, total);
    const uint32_t p11 = load_rgb(frames, row1 + x1 * 3, total);
    uint32_t v = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = chan(p00, c) + (chan(p01, c) - chan(p00, c)) * fx;
      const float bot = chan(p10, c) + (chan(p11, c) - chan(p10, c)) * fx;
      const float q = fminf(fmaxf(rintf(top + (bot - top) * fy), 0.f), 255.f);
      v |= (uint32_t)q << (8 * c);
    }
    px[i] = v;
  }
  out[0] = px[0] | (px[1] << 24);
  out[1] = (px[1] >> 8) | (px[2] << 16);
  out[2] = (px[2] >> 16) | (px[3] << 8);
}

}  // namespace aiko

// frames uint8 [B, H, W, 3] (>= 4 bytes), det fp32 [B, max_det, 6], count int32 [B] ->
// crops uint8 [B*K, Ho, Wo, 3] (4-byte aligned), rois int32 [B*K, 4] (16-byte aligned)
extern "C" int aiko_roi_crop_u8(const void* frames, const float* det, const int* count, void* crops,
                                int* rois, int B, int H, int W, int max_det, int K, int Ho, int Wo,
                                float margin, hipStream_t stream) {
  if (B < 1 || H < 1 || W < 1 || K < 1 || K > max_det || Ho < 1 || Wo < 4 || Wo % 4 || !(margin >= 0.f))
    return -1;
  const long total = (long)B * H * W * 3;
  const long slots = (long)B * K, threads = (long)Ho * (Wo / 4);
  if (total < 4 || slots > 65535 || threads > (1L << 30) || W > (1 << 24) || H > (1 << 24)) return -1;
  if (reinterpret_cast<uintptr_t>(crops) % 4 || reinterpret_cast<uintptr_t>(rois) % 16) return -1;
  const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)slots);
  aiko::roi_crop_u8_kernel<<<grid, 256, 0, stream>>>(static_cast<const uint8_t*>(frames), det, count,
                                                     static_cast<uint8_t*>(crops), rois, H, W, max_det,
                                                     K, Ho, Wo, margin, total);
  return (int)hipGetLastError();
}
