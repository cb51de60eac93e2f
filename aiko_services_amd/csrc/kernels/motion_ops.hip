// Motion detection (gfx950): did anything change in a fixed camera's view, and where?  uint8 RGB
// frames [B, H, W, 3] (batch row b is camera b) against a per-camera background of cell means that
// stays in HBM between frames, -> the moving regions in the detector's own row format (``det``
// [B, max_det, 6] + ``count`` [B], detect_ops.hip), so the tracker, the overlay, the redaction and
// the ROI crop work behind it unchanged.  Two launches per step, no host copy, no synchronisation.
// The rule is stated in ops/motion.py; it is all integer except one fp64 division, and
// ops/reference.py motion_detect_ref gives the same bits.
//
//   * motion_cells_kernel: the memory-bound part.  Every pixel is read once; per cell of ``cell`` x
//     ``cell`` pixels (8, 16 or 32, anchored at the frame's origin: the mosaic's grid of
//     redact_ops.hip) the luma mean in sixteenths is set against the background, which moves
//     towards it.  Only the background and one byte per cell are written.  The cell sums are the
//     segmented reduction of redact_ops.hip: a thread's 16 pixels lie in one cell, xor-shuffles
//     combine the lanes of a wave that share it, the 1, 2 or 4 waves of a cell meet in LDS.
//   * motion_regions_kernel: one workgroup per frame labels the 8-connected components of the
//     moving cells in LDS and writes the largest as rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aiko_api.h"

namespace aiko {

constexpr int MO_TW = 128, MO_TH = 32;               // pixels per tile: one workgroup (RD_TW, RD_TH)
constexpr int MO_THREADS = 256;
constexpr int MO_WAVES = MO_THREADS / 64;
constexpr int MO_TPR = MO_TW / 4;                     // threads per tile row, 4 adjacent pixels each
constexpr int MO_WROWS = MO_TH / MO_WAVES;            // consecutive tile rows owned by one wave
constexpr int MO_PSTEP = 64 / MO_TPR;                 // rows a wave covers per pass
constexpr int MO_PASSES = MO_WROWS / MO_PSTEP;        // passes: rows py, py + MO_PSTEP, ...
constexpr int MO_CELLS = (MO_TW / 8) * (MO_TH / 8);   // cells of a tile at the smallest cell
static_assert(MO_PASSES == 4 && MO_TPR == 32 && MO_WROWS == 8 && MO_CELLS == 64,
              "lane -> pixel map and the cell tables below");

constexpr int MO_MAX_SIDE = 255;                      // cells per grid row and per grid column
constexpr int MO_MAX_CELLS = 16384;                   // cells per frame
constexpr int MO_MAX_DET = 64;
constexpr int RG_THREADS = 1024;
constexpr int RG_WAVES = RG_THREADS / 64;
// the grid with a border of one cell all round: (Gh + 2) (Gw + 2) <= Gh Gw + 2 (Gh + Gw) + 4 and,
// with Gh Gw <= 16384 and both sides <= 255, Gh + Gw <= 255 + 65
constexpr int RG_PAD = MO_MAX_CELLS + 2 * (MO_MAX_SIDE + 65) + 4;
constexpr uint16_t RG_NONE = 0xffffu;                 // the label of a cell that does not move
static_assert(RG_PAD < 0x7fff, "labels are 16 bits, the selection key keeps 15 for them");
static_assert(MO_MAX_CELLS < (1 << 15), "the selection key is area << 15 | label in an int");

struct MotionCellArgs {
  const uint8_t* frames;
  const int* bg;                // [B, Gh, Gw]
  const int* seen;              // [B]
  int* bg_out;
  int* seen_out;
  uint8_t* mask;                // [B, Gh, Gw]
  int H, W, Gh, Gw;
  int lgc;                      // log2(cell): 3..5
  int thr16;                    // 16 * threshold
  int shift, half;              // learn_shift and its rounding term
  int learn_moving, warmup;
};

// (77 R + 150 G + 29 B + 128) >> 8 of R | G << 8 | B << 16: one byte-wise dot product with the
// coefficients 77 | 150 << 8 | 29 << 16 on top of the rounding term
__device__ __forceinline__ uint32_t mo_luma(uint32_t rgb) {
  return __builtin_amdgcn_udot4(rgb, 0x001d964du, 128u, false) >> 8;
}

// Grid (tiles x, tiles y, B), one MO_TW x MO_TH tile per workgroup; a thread owns 4 adjacent pixels
// in each of MO_PASSES rows, a wave a strip of MO_WROWS rows (the layout of redact_ops.hip).  Every
// cell size divides both tile sides, so no cell straddles two workgroups: no atomics, nothing zeroed.
// VEC: W % 4 == 0 and frames 4-byte aligned, so a thread's 4 pixels are three aligned dwords.
template <bool VEC>
__global__ __launch_bounds__(MO_THREADS) void motion_cells_kernel(const MotionCellArgs a) {
  __shared__ uint32_t s_part[MO_WAVES * (MO_TPR / 2)];     // [wave][cell column]: luma sums

  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * MO_TW, ty0 = blockIdx.y * MO_TH;
  const int tx1 = min(tx0 + MO_TW, a.W), ty1 = min(ty0 + MO_TH, a.H);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid % MO_TPR;                       // this thread's group of 4 pixels in the tile row
  const int px = tx0 + col * 4;                       // the first of them
  const int py = ty0 + wave * MO_WROWS + lane / MO_TPR;    // this thread's row in pass 0
  const long frame = (long)b * a.H;

  uint32_t sum = 0;                                   // luma of this thread's in-frame pixels
#pragma unroll
  for (int p = 0; p < MO_PASSES; ++p) {
    const int y = py + p * MO_PSTEP;
    if (y >= ty1 || px >= tx1) continue;
    const long off = ((frame + y) * a.W + px) * 3;
    if (VEC) {                                        // px + 3 < W: both are multiples of 4
      const uint32_t* q = reinterpret_cast<const uint32_t*>(a.frames + off);
      const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
      sum += mo_luma(d0 & 0xffffffu) + mo_luma((d0 >> 24) | ((d1 & 0xffffu) << 8)) +
             mo_luma((d1 >> 16) | ((d2 & 0xffu) << 16)) + mo_luma(d2 >> 8);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (px + i < tx1) {
          const uint8_t* q = a.frames + off + 3 * i;
          sum += mo_luma((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16));
        }
    }
  }
  const int s = max(a.seen[b], 0);                    // in flight with the pixels

  const int lgc = a.lgc;
  const int lg = lgc - 2;                             // log2(threads of a row per cell)
  sum += __shfl_xor(sum, 32);                         // the other row of each pass
  for (int d = 1; d < (1 << lg); d <<= 1) sum += __shfl_xor(sum, d);      // the neighbours in the row
  if (lane < MO_TPR && (col & ((1 << lg) - 1)) == 0) s_part[wave * (MO_TPR / 2) + (col >> lg)] = sum;
  __syncthreads();

  // one thread per cell: the sums of its waves, the pixel count from the frame's size
  const int lcx = 7 - lgc;                            // log2(cells per tile row)
  if (tid < (MO_TW * MO_TH) >> (2 * lgc)) {
    const int cx = tid & ((1 << lcx) - 1), cy = tid >> lcx;
    const int gx = (tx0 >> lgc) + cx, gy = (ty0 >> lgc) + cy;
    if (gx < a.Gw && gy < a.Gh) {
      const int nw = 1 << (lgc - 3), w0 = cy << (lgc - 3);
      uint32_t S = 0;
      for (int w = 0; w < nw; ++w) S += s_part[(w0 + w) * (MO_TPR / 2) + cx];
      const int nx = min(1 << lgc, a.W - (gx << lgc)), ny = min(1 << lgc, a.H - (gy << lgc));
      const uint32_t n = (uint32_t)(nx * ny);         // >= 1: the cell starts inside the frame
      const int cur = (int)((32u * S + n) / (2u * n));
      const long cell = ((long)b * a.Gh + gy) * a.Gw + gx;
      const int bg = a.bg[cell];
      const long d = (long)cur - (long)bg;            // a garbage background must not overflow
      const bool moving = s >= a.warmup && (d < 0 ? -d : d) > (long)a.thr16;
      int nb;
      if (s == 0)
        nb = cur;
      else if (moving && !a.learn_moving)
        nb = bg;
      else
        nb = (int)((long)bg + ((d + (long)a.half) >> a.shift));
      a.bg_out[cell] = nb;
      a.mask[cell] = moving ? 1 : 0;
    }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) a.seen_out[b] = s == INT32_MAX ? s : s + 1;
}

struct MotionRegionArgs {
  const uint8_t* mask;          // [B, Gh, Gw]
  float* det;                   // [B, max_det, 6]
  int* count;                   // [B]
  int* cells;                   // [B]
  int H, W, Gh, Gw;
  int lgc, min_cells, max_det;
};

__device__ __forceinline__ int rg_wave_max(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}

// Grid B, one workgroup per frame.  The labels live in LDS on the grid with a border of one cell
// that never moves, so a cell's eight neighbours are eight fixed offsets; a label is the (padded)
// index of a cell of the same component, which orders cells as the raster index does.
//   1. label = own index.  Then rounds: every moving cell takes the minimum label of its 3 x 3
//      neighbourhood, then follows label = label[label] to a fixed point.  Labels only fall and only
//      to labels of the same component, so whatever the interleaving of the threads, a round that
//      changes nothing has every cell at its component's smallest index.  The rounds are counted:
//      a chain of n cells needs fewer than n.
//   2. area per label by integer LDS atomics (order-independent), a wave whose cells share a label
//      adds once.
//   3. at most max_det selection rounds: workgroup arg-max over (area, lower label first), then the
//      box of that label by a min / max reduction.
// Threads race only as readers of a 16-bit label another thread is lowering; both values are valid.
__global__ __launch_bounds__(RG_THREADS) void motion_regions_kernel(const MotionRegionArgs a) {
  __shared__ uint16_t s_label[RG_PAD];
  __shared__ int s_area[RG_PAD];
  __shared__ int s_red[RG_WAVES];
  __shared__ int s_box[RG_WAVES][4];
  __shared__ int s_cells;

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Gh = a.Gh, Gw = a.Gw, Wp = Gw + 2;
  const int np = (Gh + 2) * Wp;                       // <= RG_PAD
  volatile uint16_t* label = s_label;

  for (int p = tid; p < np; p += RG_THREADS) {
    s_label[p] = RG_NONE;
    s_area[p] = 0;
  }
  if (tid == 0) s_cells = 0;
  __syncthreads();
  int moving = 0;
  const uint8_t* m = a.mask + (long)b * Gh * Gw;
  for (int gy = wave; gy < Gh; gy += RG_WAVES)
    for (int gx = lane; gx < Gw; gx += 64)
      if (m[gy * Gw + gx]) {
        const int p = (gy + 1) * Wp + gx + 1;
        s_label[p] = (uint16_t)p;
        ++moving;
      }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) moving += __shfl_xor(moving, d);
  if (lane == 0 && moving) atomicAdd(&s_cells, moving);
  __syncthreads();
  const int total = s_cells;                          // uniform

  if (total > 0) {
    for (int round = 0; round < np; ++round) {        // counted: ends by itself whatever the LDS holds
      int changed = 0;
      for (int p = tid; p < np; p += RG_THREADS) {
        const int own = label[p];
        if (own == RG_NONE) continue;                 // the border too
        int v = own;
        v = min(v, label[p - Wp - 1]); v = min(v, label[p - Wp]); v = min(v, label[p - Wp + 1]);
        v = min(v, label[p - 1]);                                 v = min(v, label[p + 1]);
        v = min(v, label[p + Wp - 1]); v = min(v, label[p + Wp]); v = min(v, label[p + Wp + 1]);
        if (v < own) {
          label[p] = (uint16_t)v;
          changed = 1;
        }
      }
      __syncthreads();
      for (int p = tid; p < np; p += RG_THREADS) {
        int l = label[p];
        if (l == RG_NONE) continue;
        for (int hop = 0; hop < np; ++hop) {          // strictly falling: fewer than np hops
          const int ll = label[l];
          if (ll >= l) break;
          l = ll;
        }
        label[p] = (uint16_t)l;
      }
      if (!__syncthreads_or(changed)) break;
    }

    for (int p0 = 0; p0 < np; p0 += RG_THREADS) {     // uniform trip count: the ballots below
      const int p = p0 + tid;
      const uint16_t l = p < np ? s_label[p] : RG_NONE;
      const bool on = l != RG_NONE;
      const unsigned long long act = __ballot(on);
      if (!act) continue;
      const int first = __ffsll((long long)act) - 1;
      const uint16_t l0 = (uint16_t)__shfl((int)l, first);
      if (__ballot(on && l != l0) == 0ull) {
        if (lane == first) atomicAdd(&s_area[l0], __popcll(act));
      } else if (on) {
        atomicAdd(&s_area[l], 1);
      }
    }
    __syncthreads();
  }

  float* rows = a.det + (long)b * a.max_det * 6;
  int n = 0;                                          // rows written so far: uniform
  for (; n < a.max_det && total > 0; ++n) {
    int key = 0;                                      // area << 15 | (0x7fff - label): only a root has an area
    for (int p = tid; p < np; p += RG_THREADS) {
      const int ar = s_area[p];
      if (ar >= a.min_cells) key = max(key, (ar << 15) | (0x7fff - p));
    }
    key = rg_wave_max(key);
    if (lane == 0) s_red[wave] = key;
    __syncthreads();
    key = 0;
#pragma unroll
    for (int w = 0; w < RG_WAVES; ++w) key = max(key, s_red[w]);
    if (key == 0) break;                              // uniform: nothing qualifies any more
    const int sel = 0x7fff - (key & 0x7fff), area = key >> 15;
    int x0 = Gw, y0 = Gh, x1 = -1, y1 = -1;           // as max of the negated minimum
    for (int gy = wave; gy < Gh; gy += RG_WAVES)
      for (int gx = lane; gx < Gw; gx += 64)
        if (s_label[(gy + 1) * Wp + gx + 1] == sel) {
          x0 = min(x0, gx); y0 = min(y0, gy);
          x1 = max(x1, gx); y1 = max(y1, gy);
        }
    x0 = -rg_wave_max(-x0); y0 = -rg_wave_max(-y0);
    x1 = rg_wave_max(x1); y1 = rg_wave_max(y1);
    if (lane == 0) {
      s_box[wave][0] = x0; s_box[wave][1] = y0; s_box[wave][2] = x1; s_box[wave][3] = y1;
    }
    __syncthreads();                                  // every thread has read s_red and s_area by now
    if (tid == 0) {
      s_area[sel] = 0;                                // taken
      for (int w = 0; w < RG_WAVES; ++w) {
        x0 = min(x0, s_box[w][0]); y0 = min(y0, s_box[w][1]);
        x1 = max(x1, s_box[w][2]); y1 = max(y1, s_box[w][3]);
      }
      float* row = rows + n * 6;
      row[0] = (float)(x0 << a.lgc);
      row[1] = (float)(y0 << a.lgc);
      row[2] = (float)min((x1 + 1) << a.lgc, a.W);
      row[3] = (float)min((y1 + 1) << a.lgc, a.H);
      row[4] = (float)((double)area / (double)((x1 - x0 + 1) * (y1 - y0 + 1)));
      row[5] = 0.f;
    }
    __syncthreads();                                  // s_area, s_box before the next round
  }
  for (int i = n * 6 + tid; i < a.max_det * 6; i += RG_THREADS) rows[i] = 0.f;
  if (tid == 0) {
    a.count[b] = n;
    a.cells[b] = total;
  }
}

}  // namespace aiko

namespace {

// log2(cell) and the grid, or false for a geometry the launches do not cover
bool motion_grid(int B, int H, int W, int cell, int& lgc, int& Gh, int& Gw) {
  lgc = 0;
  for (int l = 3; l <= 5; ++l)
    if (cell == 1 << l) lgc = l;
  if (!lgc || B < 1 || B > 65535 || H < 1 || W < 1 || W > (1 << 24) || H > (1 << 24)) return false;
  Gh = (H + cell - 1) >> lgc;
  Gw = (W + cell - 1) >> lgc;
  return Gh <= aiko::MO_MAX_SIDE && Gw <= aiko::MO_MAX_SIDE && Gh * Gw <= aiko::MO_MAX_CELLS;
}

}  // namespace

// The three entry points return -1 for a configuration the launches do not cover.  Gh = ceil(H /
// cell), Gw = ceil(W / cell).
// The cell pass: frames uint8 [B, H, W, 3]; bg int32 [B, Gh, Gw] and seen int32 [B], in and out (out
// no alias of in); mask uint8 [B, Gh, Gw].
extern "C" int aiko_motion_cells(const void* frames, const int* bg, const int* seen, int* bg_out, int* seen_out,
                                 void* mask, int B, int H, int W, int cell, int threshold, int learn_shift,
                                 int learn_moving, int warmup, hipStream_t stream) {
  int lgc, Gh, Gw;
  if (!motion_grid(B, H, W, cell, lgc, Gh, Gw) || threshold < 0 || threshold > 255 || learn_shift < 0 ||
      learn_shift > 8 || warmup < 1)
    return -1;
  const long tiles_x = (W + aiko::MO_TW - 1) / aiko::MO_TW, tiles_y = (H + aiko::MO_TH - 1) / aiko::MO_TH;
  aiko::MotionCellArgs c;
  c.frames = static_cast<const uint8_t*>(frames);
  c.bg = bg; c.seen = seen; c.bg_out = bg_out; c.seen_out = seen_out;
  c.mask = static_cast<uint8_t*>(mask);
  c.H = H; c.W = W; c.Gh = Gh; c.Gw = Gw;
  c.lgc = lgc;
  c.thr16 = 16 * threshold;
  c.shift = learn_shift;
  c.half = learn_shift ? 1 << (learn_shift - 1) : 0;
  c.learn_moving = learn_moving ? 1 : 0;
  c.warmup = warmup;
  const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)B);     // Gh <= 255: at most 255 tile rows
  if (W % 4 == 0 && reinterpret_cast<uintptr_t>(frames) % 4 == 0)
    aiko::motion_cells_kernel<true><<<grid, aiko::MO_THREADS, 0, stream>>>(c);
  else
    aiko::motion_cells_kernel<false><<<grid, aiko::MO_THREADS, 0, stream>>>(c);
  return (int)hipGetLastError();
}

// The region pass: mask uint8 [B, Gh, Gw] -> det fp32 [B, max_det, 6], count int32 [B], cells int32 [B].
extern "C" int aiko_motion_regions(const void* mask, float* det, int* count, int* cells, int B, int H, int W, int cell,
                                   int min_cells, int max_det, hipStream_t stream) {
  int lgc, Gh, Gw;
  if (!motion_grid(B, H, W, cell, lgc, Gh, Gw) || min_cells < 1 || max_det < 1 || max_det > aiko::MO_MAX_DET)
    return -1;
  aiko::MotionRegionArgs r;
  r.mask = static_cast<const uint8_t*>(mask);
  r.det = det; r.count = count; r.cells = cells;
  r.H = H; r.W = W; r.Gh = Gh; r.Gw = Gw;
  r.lgc = lgc; r.min_cells = min_cells; r.max_det = max_det;
  aiko::motion_regions_kernel<<<dim3((unsigned)B), aiko::RG_THREADS, 0, stream>>>(r);
  return (int)hipGetLastError();
}

// One step: both passes on ``stream``, nothing launched unless both are covered.
extern "C" int aiko_motion_detect(const void* frames, const int* bg, const int* seen, int* bg_out, int* seen_out,
                                  float* det, int* count, void* mask, int* cells, int B, int H, int W, int cell,
                                  int threshold, int learn_shift, int learn_moving, int warmup, int min_cells,
                                  int max_det, hipStream_t stream) {
  if (min_cells < 1 || max_det < 1 || max_det > aiko::MO_MAX_DET) return -1;
  const int rc = aiko_motion_cells(frames, bg, seen, bg_out, seen_out, mask, B, H, W, cell, threshold, learn_shift,
                                   learn_moving, warmup, stream);
  return rc ? rc : aiko_motion_regions(mask, det, count, cells, B, H, W, cell, min_cells, max_det, stream);
}
