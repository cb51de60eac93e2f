// Detection redaction (gfx950): the pixels inside the boxes of the detector's fixed-size NMS output
// (``det`` [B, max_det, 6] + ``count`` [B], detect_ops.hip; optionally a class per ROI slot and a
// table of the classes to hide) replaced by a mosaic or a flat colour, in uint8 frames on the
// device.  Rows and counts are read by the kernel, so a frame is redacted by one graph-replayable
// launch before anything leaves the device.  The rule is stated in ops/redact.py.
//
// The mosaic's cells are ``block`` x ``block`` pixels anchored at the frame's origin, block in
// {4, 8, 16, 32}: every cell lies in one tile (the tile sides are multiples of 32), so a workgroup
// reads every pixel its cells need before it writes any and redacting in place (out == frames) is
// safe.  All arithmetic is integer except the rect (roi_rect.h, the rect of roi_crop).
//
// Cell sums are a segmented reduction, not LDS atomics: a thread's 16 pixels lie in one cell (two at
// block 4), the lanes of a wave that share a cell are combined by xor-shuffles (red and blue packed
// in one register: a wave's share of a cell is at most 256 pixels, 16 bits per channel), and the
// 1, 2 or 4 waves of a cell meet in the thread that divides.  Nothing has to be zeroed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "roi_rect.h"
#include "aiko_api.h"

namespace aiko {

constexpr int RD_TW = 128, RD_TH = 32;               // pixels per tile: one workgroup
constexpr int RD_THREADS = 256;
constexpr int RD_WAVES = RD_THREADS / 64;
constexpr int RD_TPR = RD_TW / 4;                     // threads per tile row, 4 adjacent pixels each
constexpr int RD_WROWS = RD_TH / RD_WAVES;            // consecutive tile rows owned by one wave
constexpr int RD_PSTEP = 64 / RD_TPR;                 // rows a wave covers per pass
constexpr int RD_PASSES = RD_WROWS / RD_PSTEP;        // passes: rows py, py + RD_PSTEP, ...
constexpr int RD_CHUNK = RD_THREADS;                  // detection rows culled per round, one per thread
constexpr int RD_CELLS = (RD_TW / 4) * (RD_TH / 4);   // cells of a tile at the smallest block
constexpr uint32_t RD_ALL = 0xffffu;                  // one bit per pixel of a thread
static_assert(RD_PASSES == 4 && RD_TPR == 32 && RD_WROWS == 8 && RD_CELLS == RD_THREADS,
              "covered mask, lane -> pixel map and the cell tables below");

struct RedactArgs {
  const uint8_t* frames;
  uint8_t* out;
  const float* det;
  const int* count;
  const int* labels;            // [B*K] or null: the class is (int)det[b, i, 5]
  const uint8_t* select;        // [C] or null: every class is selected
  int H, W, max_det, K, C;
  int lgb;                      // log2(block): 2..5; pixelate only
  int pixelate;                 // 0: fill
  uint32_t fill;                // R | G << 8 | B << 16
  float margin;
  int in_place;
};

// Bits k = 0..3 set iff a <= px + k < b.
__device__ __forceinline__ uint32_t rd_range4(int a, int b, int px) {
  const int lo = min(max(a - px, 0), 4), hi = min(max(b - px, 0), 4);
  return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// Grid (tiles x, tiles y, B), one RD_TW x RD_TH tile per workgroup; a thread owns 4 adjacent pixels
// in each of RD_PASSES rows, a wave a strip of RD_WROWS rows (the layout of overlay_ops.hip).  Per
// round of RD_CHUNK rows every thread takes one used row of the frame and keeps it iff its rect
// touches the tile and its class is selected; a wave ballot compacts the kept rects into LDS and
// every thread ORs them into its 16-bit covered mask (a rect that holds the whole tile fills every
// mask at once).  A tile that kept nothing is a plain copy (nothing at all in place).  Otherwise
// the cell colours are computed from all of the tile's pixels and the covered ones take them.
// Out of place the pixels are loaded before the cull, so its chain of dependent loads (count, row,
// class, select) overlaps with theirs.
// VEC: W % 4 == 0 and both tensors 4-byte aligned, so a thread's 4 pixels are three aligned dwords.
template <bool VEC>
__global__ __launch_bounds__(RD_THREADS) void redact_detections_kernel(const RedactArgs a) {
  __shared__ int4 s_rect[RD_CHUNK];                   // X0, Y0, X1, Y1
  __shared__ uint2 s_part[RD_CELLS];                  // [wave][half][cell column]: red | blue << 16, green
  __shared__ uint32_t s_cell[RD_CELLS];               // [cell row][cell column]: the cell's colour
  __shared__ int s_wcnt[RD_WAVES], s_wfull[RD_WAVES];

  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * RD_TW, ty0 = blockIdx.y * RD_TH;
  const int tx1 = min(tx0 + RD_TW, a.W), ty1 = min(ty0 + RD_TH, a.H);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid % RD_TPR;                       // this thread's group of 4 pixels in the tile row
  const int px = tx0 + col * 4;                       // the first of them
  const int sy0 = ty0 + wave * RD_WROWS;              // the wave's strip
  const int py = sy0 + lane / RD_TPR;                 // this thread's row in pass 0; pass p adds p * RD_PSTEP
  const long frame = (long)b * a.H;

  uint32_t pix[RD_PASSES][4];                         // RGB in the low 24 bits
  uint32_t oob = 0;                                   // pixels outside the frame
#pragma unroll
  for (int p = 0; p < RD_PASSES; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pix[p][i] = 0;                                  // adds nothing to a cell's sum
      if (py + p * RD_PSTEP >= ty1 || px + i >= tx1) oob |= 1u << (4 * p + i);
    }
  uint32_t done = oob;                                // covered, or outside the frame

  auto load = [&]() {
#pragma unroll
    for (int p = 0; p < RD_PASSES; ++p) {
      const int y = py + p * RD_PSTEP;
      const long off = ((frame + y) * a.W + px) * 3;
      if (VEC) {
        if (!((oob >> (4 * p)) & 1u)) {
          const uint32_t* q = reinterpret_cast<const uint32_t*>(a.frames + off);
          const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
          pix[p][0] = d0 & 0xffffffu;
          pix[p][1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
          pix[p][2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
          pix[p][3] = d2 >> 8;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (!((oob >> (4 * p + i)) & 1u)) {
            const uint8_t* q = a.frames + off + 3 * i;
            pix[p][i] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
          }
      }
    }
  };

  if (!a.in_place) load();                            // needed whatever the rows say: in flight during the cull
  const int n = min(max(a.count[b], 0), a.K);         // used rows of this frame
  bool any = false;                                   // workgroup-uniform: some round kept a row

  for (int c0 = 0; c0 < n; c0 += RD_CHUNK) {
    const int i = c0 + tid;
    bool keep = false, full = false;
    RoiRect r{0, 0, 0, 0};
    if (i < n) {
      const float* row = a.det + ((long)b * a.max_det + i) * 6;
      const float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
      if (isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2)) {
        r = roi_rect(x1, y1, x2, y2, a.margin, a.H, a.W);
        if (r.x0 < tx1 && r.x1 > tx0 && r.y0 < ty1 && r.y1 > ty0) {      // most rows end here, class unread
          keep = true;
          if (a.select) {
            const int cls = a.labels ? a.labels[(long)b * a.K + i] : (int)row[5];   // NaN -> 0, saturating
            keep = cls >= 0 && cls < a.C && a.select[cls] != 0;
          }
          full = keep && r.x0 <= tx0 && r.x1 >= tx1 && r.y0 <= ty0 && r.y1 >= ty1;
        }
      }
    }
    // compaction: wave w holds rows c0 + 64 w ..., a lane's place is the number of kept rows in
    // front of it
    const unsigned long long m = __ballot(keep);
    const unsigned long long mf = __ballot(full);
    if (lane == 0) {
      s_wcnt[wave] = __popcll(m);
      s_wfull[wave] = mf != 0ull;
    }
    __syncthreads();
    int base = 0, total = 0, fulls = 0;
#pragma unroll
    for (int w = 0; w < RD_WAVES; ++w) {
      const int c = s_wcnt[w];
      base += w < wave ? c : 0;
      total += c;
      fulls += s_wfull[w];
    }
    if (keep) s_rect[base + __popcll(m & ((1ull << lane) - 1ull))] = make_int4(r.x0, r.y0, r.x1, r.y1);
    __syncthreads();

    any = any || total > 0;
    if (fulls) done = RD_ALL;                         // the tile lies inside one kept rect: no walk
    for (int e = 0; e < total && done != RD_ALL; ++e) {
      const int4 rc = s_rect[e];
      if (rc.y >= sy0 + RD_WROWS || rc.w <= sy0) continue;               // misses the wave's strip
      const uint32_t mx = rd_range4(rc.x, rc.z, px);                     // the 4 columns once,
      if (!mx) continue;
#pragma unroll
      for (int p = 0; p < RD_PASSES; ++p) {                              // then one nibble per pass
        const int y = py + p * RD_PSTEP;
        done |= (y >= rc.y && y < rc.w ? mx : 0u) << (4 * p);
      }
    }
    __syncthreads();                                  // the list is rewritten by the next round
  }

  if (!any) {                                         // nothing to hide in this tile
    if (a.in_place) return;
  } else if (a.in_place) {
    load();
  }
  const uint32_t hit = done & ~oob;

  if (any && a.pixelate) {
    const int lgb = a.lgb;
    const int lg = lgb - 2;                           // log2(threads of a row per cell)
    // this thread's pixels: one cell, or at block 4 one for passes 0, 1 and one for passes 2, 3
    uint32_t rb0 = 0, g0 = 0, rb1 = 0, g1 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rb0 += (pix[0][i] & 0xff00ffu) + (pix[1][i] & 0xff00ffu);
      g0 += ((pix[0][i] >> 8) & 0xffu) + ((pix[1][i] >> 8) & 0xffu);
      rb1 += (pix[2][i] & 0xff00ffu) + (pix[3][i] & 0xff00ffu);
      g1 += ((pix[2][i] >> 8) & 0xffu) + ((pix[3][i] >> 8) & 0xffu);
    }
    if (lgb > 2) {
      rb0 += rb1;
      g0 += g1;
    }
    // the other row of each pass, then the neighbours in the row that share the cell
    rb0 += __shfl_xor(rb0, 32);
    g0 += __shfl_xor(g0, 32);
    if (lgb == 2) {
      rb1 += __shfl_xor(rb1, 32);
      g1 += __shfl_xor(g1, 32);
    }
    for (int s = 1; s < (1 << lg); s <<= 1) {
      rb0 += __shfl_xor(rb0, s);
      g0 += __shfl_xor(g0, s);
    }
    if (lane < RD_TPR && (col & ((1 << lg) - 1)) == 0) {
      s_part[wave * 64 + (col >> lg)] = make_uint2(rb0, g0);
      if (lgb == 2) s_part[wave * 64 + 32 + col] = make_uint2(rb1, g1);
    }
    __syncthreads();
    // one thread per cell: the sums of its waves, the pixel count from the frame's size
    const int lcx = 7 - lgb;                          // log2(cells per tile row)
    if (tid < (RD_TW * RD_TH) >> (2 * lgb)) {
      const int cx = tid & ((1 << lcx) - 1), cy = tid >> lcx;
      uint32_t R = 0, G = 0, Bl = 0;
      if (lgb == 2) {
        const uint2 v = s_part[(cy >> 1) * 64 + (cy & 1) * 32 + cx];
        R = v.x & 0xffffu; Bl = v.x >> 16; G = v.y;
      } else {
        const int nw = 1 << (lgb - 3), w0 = cy << (lgb - 3);
        for (int w = 0; w < nw; ++w) {
          const uint2 v = s_part[(w0 + w) * 64 + cx];
          R += v.x & 0xffffu; Bl += v.x >> 16; G += v.y;
        }
      }
      const int nx = min(1 << lgb, a.W - (tx0 + (cx << lgb))), ny = min(1 << lgb, a.H - (ty0 + (cy << lgb)));
      uint32_t c = 0;
      if (nx > 0 && ny > 0) {
        const uint32_t cnt = (uint32_t)(nx * ny);
        c = (2u * R + cnt) / (2u * cnt) | ((2u * G + cnt) / (2u * cnt)) << 8 | ((2u * Bl + cnt) / (2u * cnt)) << 16;
      }
      s_cell[tid] = c;
    }
    __syncthreads();
    const int cx = col >> lg;
#pragma unroll
    for (int p = 0; p < RD_PASSES; ++p) {
      const int cy = (wave * RD_WROWS + lane / RD_TPR + p * RD_PSTEP) >> lgb;
      const uint32_t c = s_cell[(cy << lcx) + cx];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((hit >> (4 * p + k)) & 1u) pix[p][k] = c;
    }
  } else if (any) {
#pragma unroll
    for (int p = 0; p < RD_PASSES; ++p)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((hit >> (4 * p + k)) & 1u) pix[p][k] = a.fill;
  }

#pragma unroll
  for (int p = 0; p < RD_PASSES; ++p) {
    const int y = py + p * RD_PSTEP;
    const long off = ((frame + y) * a.W + px) * 3;
    if (VEC) {
      if (((oob >> (4 * p)) & 1u) || (a.in_place && !((hit >> (4 * p)) & 15u))) continue;
      uint32_t* q = reinterpret_cast<uint32_t*>(a.out + off);
      q[0] = pix[p][0] | (pix[p][1] << 24);
      q[1] = (pix[p][1] >> 8) | (pix[p][2] << 16);
      q[2] = (pix[p][2] >> 16) | (pix[p][3] << 8);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t bit = 1u << (4 * p + k);
        if ((oob & bit) || (a.in_place && !(hit & bit))) continue;
        uint8_t* q = a.out + off + 3 * k;
        q[0] = (uint8_t)pix[p][k];
        q[1] = (uint8_t)(pix[p][k] >> 8);
        q[2] = (uint8_t)(pix[p][k] >> 16);
      }
    }
  }
}

}  // namespace aiko

// frames / out uint8 [B, H, W, 3] (out == frames redacts in place), det fp32 [B, max_det, 6], count
// int32 [B], labels int32 [B*K] or null, select uint8 [C] or null.  mode 0 pixelate (block in
// {4, 8, 16, 32}), 1 fill (fill_rgb = R | G << 8 | B << 16).  Returns -1 for a configuration the
// launch does not cover.
extern "C" int aiko_redact_detections(const void* frames, void* out, const float* det, const int* count,
                                      const int* labels, const void* select, int B, int H, int W, int max_det, int K,
                                      int C, int mode, int block, int fill_rgb, float margin, hipStream_t stream) {
  if (B < 1 || H < 1 || W < 1 || K < 1 || K > max_det || (select && C < 1) || mode < 0 || mode > 1 || fill_rgb < 0 ||
      fill_rgb > 0xffffff || !(margin >= 0.f) || !(margin <= 3.0e38f))
    return -1;
  int lgb = 0;
  for (int l = 2; l <= 5; ++l)
    if (block == 1 << l) lgb = l;
  if (!lgb) return -1;
  const long tiles_x = (W + aiko::RD_TW - 1) / aiko::RD_TW, tiles_y = (H + aiko::RD_TH - 1) / aiko::RD_TH;
  if (B > 65535 || tiles_y > 65535 || W > (1 << 24) || H > (1 << 24)) return -1;
  aiko::RedactArgs a;
  a.frames = static_cast<const uint8_t*>(frames);
  a.out = static_cast<uint8_t*>(out);
  a.det = det;
  a.count = count;
  a.labels = labels;
  a.select = static_cast<const uint8_t*>(select);
  a.H = H; a.W = W; a.max_det = max_det; a.K = K; a.C = C;
  a.lgb = lgb;
  a.pixelate = mode == 0 ? 1 : 0;
  a.fill = (uint32_t)fill_rgb;
  a.margin = margin;
  a.in_place = frames == out ? 1 : 0;
  const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)B);
  const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(frames) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
  if (vec)
    aiko::redact_detections_kernel<true><<<grid, aiko::RD_THREADS, 0, stream>>>(a);
  else
    aiko::redact_detections_kernel<false><<<grid, aiko::RD_THREADS, 0, stream>>>(a);
  return (int)hipGetLastError();
}
