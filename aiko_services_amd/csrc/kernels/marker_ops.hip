// Square fiducial markers (gfx950): ArUco-style markers at any rotation and under perspective in
// uint8 RGB frames [B, H, W, 3] -> the detector's own row format (``det`` [B, max_det, 6] + ``count``
// [B], detect_ops.hip; the id is the class) plus ``corners`` and ``ids``.  Three launches per step,
// no host copy, no synchronisation, no global atomics.  The rule is stated in ops/marker.py; it is
// all integer except one fp64 division, and ops/reference.py detect_markers_ref gives the same bits.
//
//   * marker_range_kernel: every pixel is read once; min and max luma of every 16 x 16 block, by the
//     segmented reduction of motion_ops.hip (a thread's 16 pixels lie in one block, xor-shuffles
//     combine the lanes of a wave that share it, the 2 waves of a block meet in LDS).
//   * marker_mask_kernel: every pixel is read again, in the same layout, and set against the range
//     of the 3 x 3 blocks around it.  A thread's 4 pixels are a nibble of the packed dark mask [B, H,
//     ceil(W / 32)] (workspace, tail bits zero), 8 lanes make a word by shuffles; the on flags of the
//     cells meet in LDS.
//   * marker_regions_kernel: one workgroup per frame labels the 8-connected components of the on
//     cells in LDS (motion_regions_kernel's scheme), picks the candidates by their boxes, and its
//     waves take the candidates in turn: corners from the packed mask, N x N samples, decode.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aiko_api.h"

namespace aiko {

constexpr int MK_TW = 128, MK_TH = 32;               // pixels per tile: one workgroup (MO_TW, MO_TH)
constexpr int MK_THREADS = 256;
constexpr int MK_WAVES = MK_THREADS / 64;
constexpr int MK_TPR = MK_TW / 4;                     // threads per tile row, 4 adjacent pixels each
constexpr int MK_WROWS = MK_TH / MK_WAVES;            // consecutive tile rows owned by one wave
constexpr int MK_PSTEP = 64 / MK_TPR;                 // rows a wave covers per pass
constexpr int MK_PASSES = MK_WROWS / MK_PSTEP;
constexpr int MK_LGB = 4;                             // log2 of a range block's side
constexpr int MK_BX = MK_TW >> MK_LGB, MK_BY = MK_TH >> MK_LGB;      // range blocks per tile
constexpr int MK_CPR = MK_TW / 4;                     // cells per tile row at the smallest cell
static_assert(MK_PASSES == 4 && MK_TPR == 32 && MK_WROWS == 8 && MK_BX == 8 && MK_BY == 2,
              "lane -> pixel maps and the block tables below");
static_assert(MK_CPR * (MK_TH / 4) == MK_THREADS, "one thread per cell of a tile at cell 4");

constexpr int MK_MAX_SIDE = 4096;                     // H, W: the sampling's intermediates fit 64 bits
constexpr int MK_MAX_PAD = 36864;                     // (Gh + 2) (Gw + 2): 72 KB of 16-bit labels
constexpr int MK_MAX_CAND = 64, MK_MAX_DET = 64;
constexpr int MR_THREADS = 1024;
constexpr int MR_WAVES = MR_THREADS / 64;
constexpr int MR_INFLIGHT = 4;                        // words of the packed mask a lane loads at a time
constexpr uint16_t MR_NONE = 0xffffu;                 // the label of a cell that is off
static_assert(MK_MAX_PAD < MR_NONE, "labels are 16 bits");
static_assert(MK_MAX_PAD <= 64 * MR_THREADS, "a thread's cells are the bits of one 64-bit word");
static_assert(MK_MAX_CAND <= 64, "the accepted candidates are placed by one wave's ballot");

// (77 R + 150 G + 29 B + 128) >> 8 of R | G << 8 | B << 16 (mo_luma of motion_ops.hip)
__device__ __forceinline__ uint32_t mk_luma(uint32_t rgb) {
  return __builtin_amdgcn_udot4(rgb, 0x001d964du, 128u, false) >> 8;
}

struct MarkerRangeArgs {
  const uint8_t* frames;
  uint32_t* range;              // [B, Rh, Rw]: lo | hi << 8
  int H, W, Rh, Rw;
};

// Grid (tiles x, tiles y, B), one MK_TW x MK_TH tile per workgroup; a thread owns 4 adjacent pixels
// in each of MK_PASSES rows, a wave a strip of MK_WROWS rows (the layout of motion_cells_kernel).
// The blocks are anchored at the origin and 16 divides both tile sides: no block straddles two
// workgroups.  VEC: W % 4 == 0 and frames 4-byte aligned, so a thread's 4 pixels are three dwords.
template <bool VEC>
__global__ __launch_bounds__(MK_THREADS) void marker_range_kernel(const MarkerRangeArgs a) {
  __shared__ uint32_t s_part[MK_WAVES * MK_BX];       // [wave][block column]: lo | hi << 8

  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * MK_TW, ty0 = blockIdx.y * MK_TH;
  const int tx1 = min(tx0 + MK_TW, a.W), ty1 = min(ty0 + MK_TH, a.H);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid % MK_TPR;
  const int px = tx0 + col * 4;
  const int py = ty0 + wave * MK_WROWS + lane / MK_TPR;
  const long frame = (long)b * a.H;

  uint32_t lo = 255u, hi = 0u;                        // over this thread's in-frame pixels
#pragma unroll
  for (int p = 0; p < MK_PASSES; ++p) {
    const int y = py + p * MK_PSTEP;
    if (y >= ty1 || px >= tx1) continue;
    const long off = ((frame + y) * a.W + px) * 3;
    if (VEC) {                                        // px + 3 < W: both are multiples of 4
      const uint32_t* q = reinterpret_cast<const uint32_t*>(a.frames + off);
      const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
      const uint32_t y0 = mk_luma(d0 & 0xffffffu), y1 = mk_luma((d0 >> 24) | ((d1 & 0xffffu) << 8));
      const uint32_t y2 = mk_luma((d1 >> 16) | ((d2 & 0xffu) << 16)), y3 = mk_luma(d2 >> 8);
      lo = min(min(lo, min(y0, y1)), min(y2, y3));
      hi = max(max(hi, max(y0, y1)), max(y2, y3));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (px + i < tx1) {
          const uint8_t* q = a.frames + off + 3 * i;
          const uint32_t v = mk_luma((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16));
          lo = min(lo, v);
          hi = max(hi, v);
        }
    }
  }
  lo = min(lo, (uint32_t)__shfl_xor((int)lo, 32));    // the other row of each pass
  hi = max(hi, (uint32_t)__shfl_xor((int)hi, 32));
#pragma unroll
  for (int d = 1; d <= 2; d <<= 1) {                  // the block's 4 threads in the row
    lo = min(lo, (uint32_t)__shfl_xor((int)lo, d));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, d));
  }
  if (lane < MK_TPR && (col & 3) == 0) s_part[wave * MK_BX + (col >> 2)] = lo | (hi << 8);
  __syncthreads();

  if (tid < MK_BX * MK_BY) {                          // one thread per block: its two waves
    const int bx = tid % MK_BX, by = tid / MK_BX;
    const int rx = (tx0 >> MK_LGB) + bx, ry = (ty0 >> MK_LGB) + by;
    if (rx < a.Rw && ry < a.Rh) {
      const uint32_t p0 = s_part[(2 * by) * MK_BX + bx], p1 = s_part[(2 * by + 1) * MK_BX + bx];
      a.range[((long)b * a.Rh + ry) * a.Rw + rx] = min(p0 & 255u, p1 & 255u) | (max(p0 >> 8, p1 >> 8) << 8);
    }
  }
}

struct MarkerMaskArgs {
  const uint8_t* frames;
  const uint32_t* range;        // [B, Rh, Rw]
  uint32_t* words;              // [B, H, Ww]: bit x % 32 of word x / 32 is pixel x
  uint8_t* mask;                // [B, Gh, Gw]
  int H, W, Rh, Rw, Ww, Gh, Gw;
  int lgc;                      // log2(cell): 2..4
  int contrast;
};

// Grid (tiles x, tiles y, B), the same tiles and the same lane -> pixel map as the range pass: a
// thread owns 4 adjacent pixels in each of MK_PASSES rows, three dwords where VEC.  A pixel is dark iff
// 2 Y < thr of its block, thr = m + M of the 3 x 3 blocks around it, or 0 where M - m < contrast.  A
// thread's 4 dark bits are a nibble of a word of the packed mask: the 8 lanes of a word or them
// together by xor-shuffles and the first stores it.  A thread's 4 pixels lie in one cell at every cell
// size: a nibble that is not zero turns its cell on in LDS (every writer stores the same 1).
template <bool VEC>
__global__ __launch_bounds__(MK_THREADS) void marker_mask_kernel(const MarkerMaskArgs a) {
  __shared__ int s_thr[MK_BX * MK_BY];
  __shared__ uint8_t s_on[MK_THREADS];                // [cell row][cell column], MK_CPR a row

  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * MK_TW, ty0 = blockIdx.y * MK_TH;
  const int tx1 = min(tx0 + MK_TW, a.W), ty1 = min(ty0 + MK_TH, a.H);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid % MK_TPR;
  const int px = tx0 + col * 4;
  const int py = ty0 + wave * MK_WROWS + lane / MK_TPR;
  const long frame = (long)b * a.H;

  // the pixels first: MK_PASSES loads in flight; R | G << 8 | B << 16 per pixel, 0 out of the frame
  uint32_t v[MK_PASSES][4];
#pragma unroll
  for (int p = 0; p < MK_PASSES; ++p) {
    const int y = py + p * MK_PSTEP;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[p][i] = 0u;
    if (y >= ty1 || px >= tx1) continue;
    const long off = ((frame + y) * a.W + px) * 3;
    if (VEC) {                                        // px + 3 < W: both are multiples of 4
      const uint32_t* q = reinterpret_cast<const uint32_t*>(a.frames + off);
      const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
      v[p][0] = d0 & 0xffffffu;
      v[p][1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
      v[p][2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
      v[p][3] = d2 >> 8;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (px + i < tx1) {
          const uint8_t* q = a.frames + off + 3 * i;
          v[p][i] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
        }
    }
  }

  s_on[tid] = 0;
  if (tid < MK_BX * MK_BY) {
    const int rx = (tx0 >> MK_LGB) + tid % MK_BX, ry = (ty0 >> MK_LGB) + tid / MK_BX;
    int thr = 0;
    if (rx < a.Rw && ry < a.Rh) {
      uint32_t m = 255u, M = 0u;
      const uint32_t* g = a.range + (long)b * a.Rh * a.Rw;
      for (int ny = max(ry - 1, 0); ny <= min(ry + 1, a.Rh - 1); ++ny)
        for (int nx = max(rx - 1, 0); nx <= min(rx + 1, a.Rw - 1); ++nx) {
          const uint32_t p = g[ny * a.Rw + nx];
          m = min(m, p & 255u);
          M = max(M, p >> 8);
        }
      if ((int)(M - m) >= a.contrast) thr = (int)(m + M);
    }
    s_thr[tid] = thr;
  }
  __syncthreads();

  const int lgc = a.lgc;
  const int thr = s_thr[(wave / (MK_WAVES / MK_BY)) * MK_BX + (col >> 2)];      // this thread's block
#pragma unroll
  for (int p = 0; p < MK_PASSES; ++p) {               // no lane leaves before the shuffles
    const int y = py + p * MK_PSTEP;
    uint32_t nib = 0u;
    if (y < ty1) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (px + i < tx1 && (int)(2u * mk_luma(v[p][i])) < thr) nib |= 1u << i;
    }
    uint32_t word = nib << (4 * (lane & 7));
#pragma unroll
    for (int d = 1; d <= 4; d <<= 1) word |= (uint32_t)__shfl_xor((int)word, d);
    if ((lane & 7) == 0 && y < ty1 && px < tx1) a.words[(frame + y) * a.Ww + (px >> 5)] = word;
    if (nib) s_on[((y - ty0) >> lgc) * MK_CPR + ((px - tx0) >> lgc)] = 1;
  }
  __syncthreads();

  const int lcx = 7 - lgc;                            // log2(cells per tile row)
  if (tid < (MK_TW * MK_TH) >> (2 * lgc)) {
    const int cx = tid & ((1 << lcx) - 1), cy = tid >> lcx;
    const int gx = (tx0 >> lgc) + cx, gy = (ty0 >> lgc) + cy;
    if (gx < a.Gw && gy < a.Gh) a.mask[((long)b * a.Gh + gy) * a.Gw + gx] = s_on[cy * MK_CPR + cx];
  }
}

struct MarkerRegionArgs {
  const uint8_t* frames;
  const uint32_t* words;        // [B, H, Ww]
  const uint8_t* mask;          // [B, Gh, Gw]
  float* det;                   // [B, max_det, 6]
  int* count;                   // [B]
  int* corners;                 // [B, max_det, 4, 2]
  int* ids;                     // [B, max_det]
  int* cands;                   // [B]
  int H, W, Ww, Gh, Gw;
  int lgc, N, contrast, min_side, max_cand, max_det;
};

__device__ __forceinline__ long long mr_wave_max(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}

__device__ __forceinline__ int mr_wave_max(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}

// (primary, lower y, lower x) as one number to maximise: |primary| <= 8190, x and y < 4096
__device__ __forceinline__ long long mr_key(int primary, int x, int y) {
  return ((long long)(primary + 8192) << 24) | (long long)((4095 - y) << 12) | (long long)(4095 - x);
}

__device__ __forceinline__ long long mr_floor_div(long long n, long long d) {      // d > 0
  const long long q = n / d;
  return q * d > n ? q - 1 : q;
}

__device__ __forceinline__ int mr_pick(const int (&v)[4], int i) {      // no indexed registers
  return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3];
}

// module (i, j) of np.rot90(bits, -r), bits the inner n x n of the N x N white ballot
__device__ __forceinline__ int mr_bit(unsigned long long white, int N, int r, int i, int j) {
  const int n = N - 2;
  const int y = r == 0 ? i : r == 1 ? n - 1 - j : r == 2 ? n - 1 - i : j;
  const int x = r == 0 ? j : r == 1 ? i : r == 2 ? n - 1 - j : n - 1 - i;
  return (int)((white >> ((y + 1) * N + x + 1)) & 1ull);
}

// Grid B, one workgroup per frame.  Dynamic LDS: s_ext uint32 [slots] | s_label uint16 [np] | s_keep
// uint16 [slots], np = (Gh + 2) (Gw + 2) the grid with a border of off cells, slots = ceil(Gh / 2)
// ceil(Gw / 2): the cells of an aligned 2 x 2 block touch each other, so it holds at most one
// component's root (the cell whose label is its own index) and a root's block is its slot.
//   1. labels: motion_regions_kernel's minimum propagation and pointer jumping; a label is the
//      padded index of the component's first cell in raster order.
//   2. boxes: three sweeps of integer LDS atomics (order-independent) on s_ext, one per extent
//      (right, left, bottom; the top is the root's row); s_keep carries the right edge, then the
//      verdict on the width.
//   3. candidates: the roots that qualify, compacted in raster order by ballot and popcount.
//   4. the waves take the candidates in turn: the rows of the box in the packed mask, a lane a
//      word, masked by the cells' labels -> eight extremes by shuffles -> the quad -> lanes 0..N^2-1
//      sample -> ballots give the border test and the bits -> decode -> the verdict in LDS.
//   5. one wave places the accepted candidates in candidate order; the rest of every output is
//      filled.
// In step 1 threads race only as readers of a 16-bit label another thread is lowering; both values
// are valid.  Every loop is counted.
__global__ __launch_bounds__(MR_THREADS) void marker_regions_kernel(const MarkerRegionArgs a) {
  extern __shared__ uint32_t s_dyn[];
  __shared__ int s_cnt[MR_WAVES];
  __shared__ int s_placed;
  __shared__ int s_cand[MK_MAX_CAND][3];              // label, first and last cell row
  __shared__ int s_res[MK_MAX_CAND][11];              // accepted, id, hi_s - lo_s, the rolled quad

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Gh = a.Gh, Gw = a.Gw, Wp = Gw + 2, lgc = a.lgc;
  const int np = (Gh + 2) * Wp;                       // <= MK_MAX_PAD
  const int Sw = (Gw + 1) >> 1, slots = ((Gh + 1) >> 1) * Sw;
  uint32_t* s_ext = s_dyn;
  uint16_t* s_label = reinterpret_cast<uint16_t*>(s_dyn + slots);
  uint16_t* s_keep = s_label + np + (np & 1);
  volatile uint16_t* label = s_label;

  for (int p = tid; p < np; p += MR_THREADS) s_label[p] = MR_NONE;
  if (tid < MK_MAX_CAND) s_res[tid][0] = 0;
  __syncthreads();
  int on = 0;
  const uint8_t* m = a.mask + (long)b * Gh * Gw;
  for (int gy = wave; gy < Gh; gy += MR_WAVES)
    for (int gx = lane; gx < Gw; gx += 64)
      if (m[gy * Gw + gx]) {
        const int p = (gy + 1) * Wp + gx + 1;
        s_label[p] = (uint16_t)p;
        ++on;
      }
  on = __syncthreads_or(on);                          // uniform: anything on at all?

  int total = 0;                                      // candidates, before the cap: uniform
  if (on) {
    // bit i: padded cell tid + i * MR_THREADS is on.  Few cells are: the sweeps below visit those only
    unsigned long long mine = 0ull;
    for (int i = 0, p = tid; p < np; ++i, p += MR_THREADS)
      if (s_label[p] != MR_NONE) mine |= 1ull << i;

    for (int round = 0; round < np; ++round) {        // counted: ends by itself whatever the LDS holds
      int changed = 0;
      for (unsigned long long left = mine; left; left &= left - 1ull) {
        const int p = tid + (__ffsll((long long)left) - 1) * MR_THREADS;
        const int own = label[p];
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
      for (unsigned long long left = mine; left; left &= left - 1ull) {
        const int p = tid + (__ffsll((long long)left) - 1) * MR_THREADS;
        int l = label[p];
        for (int hop = 0; hop < np; ++hop) {          // strictly falling: fewer than np hops
          const int ll = label[l];
          if (ll >= l) break;
          l = ll;
        }
        label[p] = (uint16_t)l;
      }
      if (!__syncthreads_or(changed)) break;
    }

    // sweep 0, 1, 2 = the right, left and bottom extent of every component, in the slot of its root
    for (int sweep = 0; sweep < 3; ++sweep) {
      for (unsigned long long left = mine; left; left &= left - 1ull) {     // the roots set up their slots
        const int p = tid + (__ffsll((long long)left) - 1) * MR_THREADS;
        if (s_label[p] == p) {
          const int gy = p / Wp - 1, gx = p % Wp - 1, slot = (gy >> 1) * Sw + (gx >> 1);
          if (sweep == 1) s_keep[slot] = (uint16_t)s_ext[slot];
          if (sweep == 2) {
            const int x0 = (int)s_ext[slot] << lgc, x1 = min(((int)s_keep[slot] + 1) << lgc, a.W);
            s_keep[slot] = x1 - x0 >= a.min_side ? 1 : 0;
          }
          s_ext[slot] = sweep == 1 ? 0xffffffffu : 0u;
        }
      }
      __syncthreads();
      for (unsigned long long left = mine; left; left &= left - 1ull) {
        const int p = tid + (__ffsll((long long)left) - 1) * MR_THREADS;
        const int l = s_label[p];
        const int ly = l / Wp - 1, lx = l % Wp - 1, slot = (ly >> 1) * Sw + (lx >> 1);
        const int gy = p / Wp - 1, gx = p % Wp - 1;
        if (sweep == 0) atomicMax(&s_ext[slot], (uint32_t)gx);
        else if (sweep == 1) atomicMin(&s_ext[slot], (uint32_t)gx);
        else atomicMax(&s_ext[slot], (uint32_t)gy);
      }
      __syncthreads();
    }

    for (int p0 = 0; p0 < np; p0 += MR_THREADS) {     // uniform trip count: the ballots and barriers below
      const int p = p0 + tid;
      bool q = false;
      int cy0 = 0, cy1 = 0;
      if (p < np && s_label[p] == p) {
        const int gx = p % Wp - 1, slot = ((p / Wp - 1) >> 1) * Sw + (gx >> 1);
        cy0 = p / Wp - 1;
        cy1 = (int)s_ext[slot];
        q = s_keep[slot] && min((cy1 + 1) << lgc, a.H) - (cy0 << lgc) >= a.min_side;
      }
      const unsigned long long act = __ballot(q);
      if (lane == 0) s_cnt[wave] = __popcll(act);
      __syncthreads();
      int before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < MR_WAVES; ++w) {
        const int c = s_cnt[w];
        before += w < wave ? c : 0;
        all += c;
      }
      const int ci = total + before + __popcll(act & ((1ull << lane) - 1ull));
      if (q && ci < a.max_cand) {
        s_cand[ci][0] = p;
        s_cand[ci][1] = cy0;
        s_cand[ci][2] = cy1;
      }
      total += all;
      __syncthreads();                                // s_cnt before the next chunk
    }
  }

  const int N = a.N, NN = N * N;
  const int ncand = min(total, a.max_cand);
  const long frame = (long)b * a.H;
  for (int ci = wave; ci < ncand; ci += MR_WAVES) {   // wave-uniform from here
    const int l = s_cand[ci][0];
    const int y0 = s_cand[ci][1] << lgc, y1 = min((s_cand[ci][2] + 1) << lgc, a.H);
    const int n = (y1 - y0) * a.Ww;                   // <= 4096 * 128
    const int ncell = 32 >> lgc;                      // cells per word
    const uint32_t cellbits = (uint32_t)((1ull << (1 << lgc)) - 1ull);
    long long key[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) key[k] = -1;
    const uint32_t* wrow = a.words + (frame + y0) * a.Ww;      // the rows of the box, one after the other
    for (int i0 = lane; i0 < n; i0 += 64 * MR_INFLIGHT) {
      uint32_t w4[MR_INFLIGHT];
#pragma unroll
      for (int k = 0; k < MR_INFLIGHT; ++k) w4[k] = i0 + 64 * k < n ? wrow[i0 + 64 * k] : 0u;
#pragma unroll
      for (int k = 0; k < MR_INFLIGHT; ++k) {
        uint32_t w = w4[k];
        if (!w) continue;
        const int i = i0 + 64 * k;
        const int y = y0 + i / a.Ww, wx = i % a.Ww;
        const uint16_t* lrow = s_label + ((y >> lgc) + 1) * Wp + 1;
        const int c0 = (wx << 5) >> lgc;
        uint32_t own = 0u;
        for (int c = 0; c < ncell; ++c)
          if (c0 + c < Gw && lrow[c0 + c] == l) own |= cellbits << (c << lgc);
        w &= own;
        if (!w) continue;
        const int xl = (wx << 5) + __ffs((int)w) - 1, xh = (wx << 5) + 31 - __clz((int)w);
        key[0] = max(key[0], mr_key(-(xl + y), xl, y));
        key[1] = max(key[1], mr_key(xh - y, xh, y));
        key[2] = max(key[2], mr_key(xh + y, xh, y));
        key[3] = max(key[3], mr_key(y - xl, xl, y));
        key[4] = max(key[4], mr_key(-y, xl, y));
        key[5] = max(key[5], mr_key(xh, xh, y));
        key[6] = max(key[6], mr_key(y, xl, y));
        key[7] = max(key[7], mr_key(-xl, xl, y));
      }
    }
    int qx[8], qy[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      key[k] = mr_wave_max(key[k]);
      qx[k] = 4095 - (int)(key[k] & 4095);
      qy[k] = 4095 - (int)((key[k] >> 12) & 4095);
    }
    if (key[0] < 0) continue;                         // no dark pixel of its own: cannot happen

    long long area[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      long long s = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        s += (long long)qx[4 * h + k] * qy[4 * h + k1] - (long long)qx[4 * h + k1] * qy[4 * h + k];
      }
      area[h] = s < 0 ? -s : s;
    }
    const bool diagonal = area[0] >= area[1];         // the diagonal quad wins a tie
    int cx[4], cy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cx[k] = diagonal ? qx[k] : qx[4 + k];
      cy[k] = diagonal ? qy[k] : qy[4 + k];
    }
    const long long x0 = cx[0], x1 = cx[1], x2 = cx[2], x3 = cx[3];
    const long long u0 = cy[0], u1 = cy[1], u2 = cy[2], u3 = cy[3];

    // rule 7: the N x N samples, lane i * N + j module (i, j)
    const long long dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 - x3;
    const long long dy1 = u1 - u2, dy2 = u3 - u2, sy = u0 - u1 + u2 - u3;
    const long long den = dx1 * dy2 - dy1 * dx2;
    if (den == 0) continue;
    const long long G = sx * dy2 - sy * dx2, Hh = dx1 * sy - dy1 * sx;
    const long long A = den * (x1 - x0) + G * x1, Bx = den * (x3 - x0) + Hh * x3;
    const long long D = den * (u1 - u0) + G * u1, E = den * (u3 - u0) + Hh * u3;
    const bool active = lane < NN;
    const int mi = active ? lane / N : 0, mj = active ? lane % N : 0;
    const long long ca = 2 * mj + 1, cb = 2 * mi + 1;
    long long dd = G * ca + Hh * cb + 2 * N * den;
    long long nx = A * ca + Bx * cb + 2 * N * den * x0;
    long long ny = D * ca + E * cb + 2 * N * den * u0;
    if (__ballot(active && dd == 0)) continue;
    if (dd < 0) {
      dd = -dd; nx = -nx; ny = -ny;
    }
    if (!active) dd = 1;
    const int spx = (int)min(max(mr_floor_div(2 * nx + dd, 2 * dd), 0ll), (long long)(a.W - 1));
    const int spy = (int)min(max(mr_floor_div(2 * ny + dd, 2 * dd), 0ll), (long long)(a.H - 1));
    int Y = 0;
    if (active) {
      const uint8_t* q = a.frames + ((frame + spy) * a.W + spx) * 3;
      Y = (int)mk_luma((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16));
    }
    const int hi_s = mr_wave_max(active ? Y : 0), lo_s = 255 - mr_wave_max(active ? 255 - Y : 0);
    if (hi_s - lo_s < a.contrast) continue;
    const bool is_white = active && 2 * Y >= lo_s + hi_s;
    const bool border = active && (mi == 0 || mi == N - 1 || mj == 0 || mj == N - 1);
    if (__ballot(border && is_white)) continue;
    const unsigned long long white = __ballot(is_white);

    // rule 8, every lane the same
    int id = -1, rot = 0;
    if (N == 7) {
      for (int r = 3; r >= 0; --r) {                  // downwards: the first that decodes stays
        bool ok = true;
        int v = 0;
        for (int i = 0; i < 5; ++i) {
          int word = 0;
          for (int j = 0; j < 5; ++j) word |= mr_bit(white, 7, r, i, j) << (4 - j);
          ok = ok && (word == 0x10 || word == 0x17 || word == 0x09 || word == 0x0e);
          v = (v << 2) | (((word >> 3) & 1) << 1) | ((word >> 1) & 1);
        }
        if (ok) {
          id = v;
          rot = r;
        }
      }
    } else {
      for (int r = 3; r >= 0; --r) {                  // downwards: the first of equal codes stays
        int code = 0;
        for (int i = 0; i < 16; ++i) code |= mr_bit(white, 6, r, i >> 2, i & 3) << i;
        if (id < 0 || code <= id) {
          id = code;
          rot = r;
        }
      }
    }
    if (id < 0) continue;
    if (lane == 0) {
      s_res[ci][1] = id;
      s_res[ci][2] = hi_s - lo_s;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int src = (k + 4 - rot) & 3;
        s_res[ci][3 + 2 * k] = mr_pick(cx, src);
        s_res[ci][4 + 2 * k] = mr_pick(cy, src);
      }
      s_res[ci][0] = 1;
    }
  }
  __syncthreads();

  float* rows = a.det + (long)b * a.max_det * 6;
  int* quads = a.corners + (long)b * a.max_det * 8;
  int* idrow = a.ids + (long)b * a.max_det;
  if (wave == 0) {                                    // lane ci places candidate ci
    const bool acc = lane < ncand && s_res[lane][0];
    const unsigned long long act = __ballot(acc);
    const int rank = __popcll(act & ((1ull << lane) - 1ull));
    if (acc && rank < a.max_det) {
      int xa = MK_MAX_SIDE, ya = MK_MAX_SIDE, xb = -1, yb = -1;
      for (int k = 0; k < 4; ++k) {
        const int x = s_res[lane][3 + 2 * k], y = s_res[lane][4 + 2 * k];
        quads[rank * 8 + 2 * k] = x;
        quads[rank * 8 + 2 * k + 1] = y;
        xa = min(xa, x); ya = min(ya, y);
        xb = max(xb, x); yb = max(yb, y);
      }
      idrow[rank] = s_res[lane][1];
      float* row = rows + rank * 6;
      row[0] = (float)xa;
      row[1] = (float)ya;
      row[2] = (float)(xb + 1);
      row[3] = (float)(yb + 1);
      row[4] = (float)((double)s_res[lane][2] / 255.0);
      row[5] = (float)s_res[lane][1];
    }
    if (lane == 0) s_placed = min(__popcll(act), a.max_det);
  }
  __syncthreads();
  const int placed = s_placed;
  for (int i = placed * 6 + tid; i < a.max_det * 6; i += MR_THREADS) rows[i] = 0.f;
  for (int i = placed * 8 + tid; i < a.max_det * 8; i += MR_THREADS) quads[i] = 0;
  for (int i = placed + tid; i < a.max_det; i += MR_THREADS) idrow[i] = -1;
  if (tid == 0) {
    a.count[b] = placed;
    a.cands[b] = total;
  }
}

}  // namespace aiko

namespace {

struct MarkerGrid {
  int lgc, Gh, Gw, Rh, Rw, Ww;
};

// the grids, or false for a geometry the launches do not cover
bool marker_grid(int B, int H, int W, int cell, MarkerGrid& g) {
  g.lgc = 0;
  for (int l = 2; l <= 4; ++l)
    if (cell == 1 << l) g.lgc = l;
  if (!g.lgc || B < 1 || B > 65535 || H < 1 || W < 1 || W > aiko::MK_MAX_SIDE || H > aiko::MK_MAX_SIDE) return false;
  g.Gh = (H + cell - 1) >> g.lgc;
  g.Gw = (W + cell - 1) >> g.lgc;
  g.Rh = (H + 15) >> aiko::MK_LGB;
  g.Rw = (W + 15) >> aiko::MK_LGB;
  g.Ww = (W + 31) >> 5;
  return (g.Gh + 2) * (g.Gw + 2) <= aiko::MK_MAX_PAD;
}

}  // namespace

// One step on ``stream``: frames uint8 [B, H, W, 3] -> det fp32 [B, max_det, 6], count int32 [B],
// corners int32 [B, max_det, 4, 2], ids int32 [B, max_det], cands int32 [B], mask uint8 [B, Gh, Gw];
// work int32 [B (H ceil(W / 32) + ceil(H / 16) ceil(W / 16))]: the packed mask, then the range grid.
// N = 7 (original) or 6 (payload16).  passes: bit 0 the range pass, bit 1 the mask pass, bit 2 the
// region pass (7: the whole step; the others are for measuring a pass alone).  Returns -1 for a
// configuration the launches do not cover; nothing is launched then.
extern "C" int aiko_marker_detect(const void* frames, float* det, int* count, int* corners, int* ids, int* cands,
                                  void* mask, void* work, int B, int H, int W, int N, int cell, int contrast,
                                  int min_side, int max_cand, int max_det, int passes, hipStream_t stream) {
  MarkerGrid g;
  if (!marker_grid(B, H, W, cell, g) || (N != 6 && N != 7) || contrast < 1 || contrast > 255 || min_side < 1 ||
      max_cand < 1 || max_cand > aiko::MK_MAX_CAND || max_det < 1 || max_det > aiko::MK_MAX_DET || passes < 1 ||
      passes > 7)
    return -1;
  uint32_t* words = static_cast<uint32_t*>(work);
  uint32_t* range = words + (long)B * H * g.Ww;
  const dim3 grid((unsigned)((W + aiko::MK_TW - 1) / aiko::MK_TW), (unsigned)((H + aiko::MK_TH - 1) / aiko::MK_TH),
                  (unsigned)B);
  const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(frames) % 4 == 0;
  if (passes & 1) {
    aiko::MarkerRangeArgs r;
    r.frames = static_cast<const uint8_t*>(frames);
    r.range = range;
    r.H = H; r.W = W; r.Rh = g.Rh; r.Rw = g.Rw;
    if (vec)
      aiko::marker_range_kernel<true><<<grid, aiko::MK_THREADS, 0, stream>>>(r);
    else
      aiko::marker_range_kernel<false><<<grid, aiko::MK_THREADS, 0, stream>>>(r);
  }
  if (passes & 2) {
    aiko::MarkerMaskArgs m;
    m.frames = static_cast<const uint8_t*>(frames);
    m.range = range; m.words = words;
    m.mask = static_cast<uint8_t*>(mask);
    m.H = H; m.W = W; m.Rh = g.Rh; m.Rw = g.Rw; m.Ww = g.Ww; m.Gh = g.Gh; m.Gw = g.Gw;
    m.lgc = g.lgc; m.contrast = contrast;
    if (vec)
      aiko::marker_mask_kernel<true><<<grid, aiko::MK_THREADS, 0, stream>>>(m);
    else
      aiko::marker_mask_kernel<false><<<grid, aiko::MK_THREADS, 0, stream>>>(m);
  }
  if (passes & 4) {
    aiko::MarkerRegionArgs r;
    r.frames = static_cast<const uint8_t*>(frames);
    r.words = words;
    r.mask = static_cast<const uint8_t*>(mask);
    r.det = det; r.count = count; r.corners = corners; r.ids = ids; r.cands = cands;
    r.H = H; r.W = W; r.Ww = g.Ww; r.Gh = g.Gh; r.Gw = g.Gw;
    r.lgc = g.lgc; r.N = N; r.contrast = contrast; r.min_side = min_side; r.max_cand = max_cand; r.max_det = max_det;
    const int np = (g.Gh + 2) * (g.Gw + 2), slots = ((g.Gh + 1) / 2) * ((g.Gw + 1) / 2);
    const size_t lds = 4ul * slots + 2ul * (np + (np & 1)) + 2ul * slots;
    if (lds > 64 * 1024) {                            // per device and function: set where it is needed
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&aiko::marker_regions_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
    }
    aiko::marker_regions_kernel<<<dim3((unsigned)B), aiko::MR_THREADS, lds, stream>>>(r);
  }
  return (int)hipGetLastError();
}
