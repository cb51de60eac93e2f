// The frame rect of one detection row, shared by roi_ops.hip (crop) and overlay_ops.hip (draw): a
// box drawn by draw_detections covers exactly the pixels roi_crop resized for the same margin.
#pragma once
#include <hip/hip_runtime.h>

namespace aiko {

struct RoiRect {
  int x0, y0, x1, y1;          // half-open, inside the frame; x1 > x0 iff the slot is valid
};

// Rect of one detection row, every operation rounded on its own so that a torch fp32 reference
// (ops/reference.py roi_rects_ref) gives the same bits:
//   bw = x2 - x1, bh = y2 - y1, ex = margin * bw, ey = margin * bh
//   fx0 = floor(x1 - ex), fx1 = ceil(x2 + ex), fy0 = floor(y1 - ey), fy1 = ceil(y2 + ey)
//   X0 = clamp(fx0, 0, W - 1), X1 = clamp(fx1, X0 + 1, W)   (in float, then to int; same for Y)
// hipcc fuses a product into a following add even through __fmul_rn / __fadd_rn (the operations in
// those header functions carry the contract flag), so the products are written with the plain
// operators under ``fp contract(off)``.
__device__ __forceinline__ RoiRect roi_rect(float x1, float y1, float x2, float y2, float margin,
                                            int H, int W) {
#pragma clang fp contract(off)
  const float bw = x2 - x1, bh = y2 - y1;
  const float ex = margin * bw, ey = margin * bh;
  const float fx0 = floorf(x1 - ex), fx1 = ceilf(x2 + ex);
  const float fy0 = floorf(y1 - ey), fy1 = ceilf(y2 + ey);
  const float X0 = fminf(fmaxf(fx0, 0.f), (float)(W - 1));
  const float X1 = fminf(fmaxf(fx1, X0 + 1.f), (float)W);
  const float Y0 = fminf(fmaxf(fy0, 0.f), (float)(H - 1));
  const float Y1 = fminf(fmaxf(fy1, Y0 + 1.f), (float)H);
  return RoiRect{(int)X0, (int)Y0, (int)X1, (int)Y1};
}

}  // namespace aiko
