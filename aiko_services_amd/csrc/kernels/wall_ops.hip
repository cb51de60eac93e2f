// Camera wall (gfx950): B uint8 frames (batch row b = camera b) reduced to P pages of R x C tiles,
// each tile the exact area average of one camera's frame, with an alert ring and the camera's
// number, in one picture that JpegEncode, RgbToYuv or FrameDownload take as it is.  Which camera a
// tile shows is decided on the device (wall_select, from an int32 score per camera such as the
// detector's counts or the motion detector's motion_cells), so the wall is two graph-replayable
// launches with no host copy between them.  The rule is stated in ops/wall.py.
//
// All arithmetic is integer.  A tile pixel is S = sum wy(i, y) wx(j, x) p[i, j] over its footprint,
// rounded once: (2 S + W H) / (2 W H).  The weights of a pixel sum to W H <= 2^23 (the launcher
// refuses more), so S <= 255 * 2^23 < 2^31 and 2 S + W H <= 510 * 2^23 + 2^23 = 511 * 2^23 < 2^32:
// unsigned 32 bits hold every intermediate.  The sum is separable: a pass first adds the source
// rows of an output row, weighted by wy, per byte column (registers -> LDS), then every output byte
// adds its columns of that image weighted by wx.  Positions are taken relative to a footprint's
// first source row / column (o F = j0 t + r), so every product below stays under 3 * 2^23.
//
// No global atomics, no scratch, every loop counted.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aiko_api.h"

namespace aiko {

constexpr int WL_THREADS = 256;
constexpr int WL_LDS = 6144;                          // dwords of column sums: rows x 3 seg <= WL_LDS
constexpr int WL_ACC = 4;                             // output bytes a thread accumulates per pass
constexpr int WL_OUT = WL_THREADS * WL_ACC;           // output bytes per pass: rows x 3 nxc <= WL_OUT
constexpr int WL_UNROLL = 4;                          // source rows in flight per thread
constexpr int WL_SEL_THREADS = 1024;
constexpr int WL_SEL_MAX = 4096;                      // cameras ranked in LDS
constexpr int WL_MAX_DIGITS = 10;

// ops/overlay_font.py, digits 0..9: one byte per glyph row, bit 7 the leftmost pixel, the 5 x 7
// design in its 6 x 8 cell (test_gpu_wall.py reads every digit back against glyph_rows)
__constant__ uint8_t wl_digits[10][8] = {
    {0x70, 0x88, 0x98, 0xa8, 0xc8, 0x88, 0x70, 0}, {0x20, 0x60, 0x20, 0x20, 0x20, 0x20, 0x70, 0},
    {0x70, 0x88, 0x08, 0x10, 0x20, 0x40, 0xf8, 0}, {0xf0, 0x08, 0x08, 0x70, 0x08, 0x08, 0xf0, 0},
    {0x10, 0x30, 0x50, 0x90, 0xf8, 0x10, 0x10, 0}, {0xf8, 0x80, 0xf0, 0x08, 0x08, 0x88, 0x70, 0},
    {0x30, 0x40, 0x80, 0xf0, 0x88, 0x88, 0x70, 0}, {0xf8, 0x08, 0x10, 0x20, 0x40, 0x40, 0x40, 0},
    {0x70, 0x88, 0x88, 0x70, 0x88, 0x88, 0x70, 0}, {0x70, 0x88, 0x88, 0x78, 0x08, 0x10, 0x60, 0}};

struct WallArgs {
  const uint8_t* frames;
  const int* score;             // [B] or null
  const int* source;            // [P * R * C]: the camera of every slot, or -1
  uint8_t* wall;
  int B, H, W, R, C, th, tw, g, Hw, Ww;
  int min_score, ring, ls, label_base;
  uint32_t bg, alert, fg, lbg;  // R | G << 8 | B << 16
  int band;                     // tile rows per workgroup, a multiple of rows
  int rows, nxc;                // output rows and columns per pass
  int seg;                      // source pixels per LDS segment, a multiple of 16
  int narrow;                   // th H and tw W fit 32 unsigned bits
};

// Footprint of output index o along a side of F source pixels reduced to t: source j0 + k for
// k < nk; source j0 + k covers [k t, (k + 1) t) and the output [r, r + F) on the same axis
struct WlSpan {
  int j0, r, nk;
};

__device__ __forceinline__ WlSpan wl_span(int o, int F, int t, int narrow) {
  WlSpan s;
  if (narrow) {
    const uint32_t a = (uint32_t)o * (uint32_t)F;
    s.j0 = (int)(a / (uint32_t)t);
    s.r = (int)(a - (uint32_t)s.j0 * (uint32_t)t);
  } else {
    // o F < 2^46 is exact in a double, and a quotient that is no integer lies at least 1 / t >=
    // 2^-23 from the next one, far more than the division's rounding: the floor is exact
    const uint64_t a = (uint64_t)o * (uint64_t)F;
    s.j0 = (int)((double)a / (double)t);
    s.r = (int)(a - (uint64_t)s.j0 * (uint64_t)t);
  }
  s.nk = (s.r + F + t - 1) / t;
  return s;
}

__device__ __forceinline__ uint32_t wl_weight(int k, int r, int F, int t) {
  return (uint32_t)(min((k + 1) * t, r + F) - max(k * t, r));
}

__device__ __forceinline__ uint32_t wl_channel(uint32_t rgb, int c) { return (rgb >> (8 * c)) & 0xffu; }

// the dword of a run of rgb pixels that starts at channel ph
__device__ __forceinline__ uint32_t wl_pattern(uint32_t rgb, int ph) {
  const uint32_t c0 = wl_channel(rgb, ph), c1 = wl_channel(rgb, ph == 2 ? 0 : ph + 1),
                 c2 = wl_channel(rgb, ph == 0 ? 2 : ph - 1);
  return c0 | c1 << 8 | c2 << 16 | c0 << 24;
}

// nrows rows of nbytes bytes (whole pixels) from byte cb0 of wall row row0 on, filled with rgb by
// the whole workgroup: one item per 16-byte aligned piece of a row, a vector store where the piece
// lies inside the row and byte stores at its two ends
__device__ void wl_fill(uint8_t* wall, long pitch, long row0, int nrows, long cb0, int nbytes, uint32_t rgb, int tid) {
  if (nrows <= 0 || nbytes <= 0) return;
  const int cpr = (nbytes + 15) / 16 + 1;
  const int items = nrows * cpr;
  for (int item = tid; item < items; item += WL_THREADS) {
    const int r = item / cpr, q = item - r * cpr;
    uint8_t* row = wall + (row0 + r) * pitch + cb0;
    const int lo = 16 * q - (int)(reinterpret_cast<uintptr_t>(row) & 15u);      // of the piece, from the row's start
    const int k0 = max(lo, 0), k1 = min(lo + 16, nbytes);
    if (k1 <= k0) continue;
    if (k1 - k0 == 16) {
      const int ph = lo % 3;
      const uint32_t p0 = wl_pattern(rgb, ph), p1 = wl_pattern(rgb, ph == 2 ? 0 : ph + 1),
                     p2 = wl_pattern(rgb, ph == 0 ? 2 : ph - 1);
      *reinterpret_cast<uint4*>(row + lo) = make_uint4(p0, p1, p2, p0);
    } else {
      for (int k = k0; k < k1; ++k) row[k] = (uint8_t)wl_channel(rgb, k % 3);
    }
  }
}

// Grid (P * R * C slots, bands of a.band tile rows).  A workgroup reads its slot's camera once,
// fills the gap above and left of its part of the tile (and right of / below the grid's last
// column / row), and, for a shown tile, walks chunks of a.nxc output columns; per chunk, passes of
// a.rows output rows:
//   phase A  an item = (output row of the pass, 16 bytes of the source segment): the source rows of
//            that output row, WL_UNROLL loads in flight, times wy into 16 registers -> LDS
//   phase B  an item = (output row, column, channel), WL_ACC per thread: the columns of its
//            footprint that lie in the segment, times wx, into a register
// and after the chunk's last segment (one, unless a single output column is wider than an LDS
// segment) the rounding, ring, label and byte store.
// VEC: W % 16 == 0 and frames 16-byte aligned, so every source row starts aligned and a segment is
// whole 16-byte loads; otherwise bytes, each checked against the row's end.
template <bool VEC>
__global__ __launch_bounds__(WL_THREADS) void wall_compose_kernel(const WallArgs a) {
  __shared__ uint4 s_v4[WL_LDS / 4];
  __shared__ int s_dig[WL_MAX_DIGITS + 1];
  uint32_t* s_v = reinterpret_cast<uint32_t*>(s_v4);

  const int tid = threadIdx.x;
  const long slot = blockIdx.x;
  const int N = a.R * a.C;
  const int t = (int)(slot % N);
  const long page = slot / N;
  const int tr = t / a.C, tc = t - tr * a.C;
  const int oy = a.g + tr * (a.th + a.g), ox = a.g + tc * (a.tw + a.g);
  const int ya = blockIdx.y * a.band, yb = min(ya + a.band, a.th);
  const bool top = blockIdx.y == 0, bottom = yb == a.th && tr == a.R - 1;
  const long pitch = (long)a.Ww * 3, prow = page * a.Hw;
  const int cellw = a.g + a.tw + (tc == a.C - 1 ? a.g : 0);           // gap, tile, the grid's right edge

  int cam = __builtin_amdgcn_readfirstlane(a.source[slot]);
  if (cam < 0 || cam >= a.B) {                                        // empty: the whole cell is background
    const int r0 = oy + ya - (top ? a.g : 0), r1 = oy + yb + (bottom ? a.g : 0);
    wl_fill(a.wall, pitch, prow + r0, r1 - r0, (long)(ox - a.g) * 3, cellw * 3, a.bg, tid);
    return;
  }
  if (top) wl_fill(a.wall, pitch, prow + oy - a.g, a.g, (long)(ox - a.g) * 3, cellw * 3, a.bg, tid);
  if (bottom) wl_fill(a.wall, pitch, prow + oy + a.th, a.g, (long)(ox - a.g) * 3, cellw * 3, a.bg, tid);
  wl_fill(a.wall, pitch, prow + oy + ya, yb - ya, (long)(ox - a.g) * 3, a.g * 3, a.bg, tid);
  if (tc == a.C - 1) wl_fill(a.wall, pitch, prow + oy + ya, yb - ya, (long)(ox + a.tw) * 3, a.g * 3, a.bg, tid);

  const bool ringed = a.ring > 0 && a.score != nullptr && __builtin_amdgcn_readfirstlane(a.score[cam]) >= a.min_score;
  int nd = 0;                                                         // digits of the label
  if (a.ls > 0) {
    uint32_t v = (uint32_t)a.label_base + (uint32_t)cam;
    uint32_t p10 = 1;
    nd = 1;
    while (v / p10 >= 10u) {                                          // at most 9 times
      p10 *= 10u;
      ++nd;
    }
    if (tid == 0) {
      for (int d = 0; d < nd; ++d) {                                  // from the left
        s_dig[d] = (int)(v / p10);
        v -= (uint32_t)s_dig[d] * p10;
        p10 /= 10u;
      }
    }
    __syncthreads();
  }
  const int boxh = 9 * a.ls, boxw = a.ls + nd * 6 * a.ls;

  const uint8_t* frame = a.frames + (long)cam * a.H * a.W * 3;
  const uint32_t WH = (uint32_t)a.W * (uint32_t)a.H;
  const int segp = a.seg * 3;                                         // dwords per row of the LDS image
  const long rowb = (long)a.W * 3;

  for (int xc0 = 0; xc0 < a.tw; xc0 += a.nxc) {
    const int nx = min(a.nxc, a.tw - xc0), nx3 = nx * 3;
    // this thread's output bytes of every pass of the chunk
    int irow[WL_ACC], icol[WL_ACC], ich[WL_ACC];
    WlSpan isp[WL_ACC];
#pragma unroll
    for (int u = 0; u < WL_ACC; ++u) {
      const int item = tid + u * WL_THREADS;
      irow[u] = item / nx3;
      const int rem = item - irow[u] * nx3;
      icol[u] = rem / 3;
      ich[u] = rem - icol[u] * 3;
      isp[u] = wl_span(xc0 + icol[u], a.W, a.tw, a.narrow);
      if (irow[u] >= a.rows) irow[u] = -1;
    }
    const WlSpan first = wl_span(xc0, a.W, a.tw, a.narrow), last = wl_span(xc0 + nx - 1, a.W, a.tw, a.narrow);
    const int jb = last.j0 + last.nk;                                 // source columns [first.j0, jb)

    for (int y0 = ya; y0 < yb; y0 += a.rows) {
      const int nr = min(a.rows, yb - y0);
      uint32_t acc[WL_ACC];
#pragma unroll
      for (int u = 0; u < WL_ACC; ++u) acc[u] = 0;

      for (int s0 = first.j0 & ~15; s0 < jb; s0 += a.seg) {
        const int sn = min(a.seg, a.W - s0), snb = sn * 3;            // the segment's pixels and bytes
        const int nq = (snb + 15) / 16;
        for (int item = tid; item < nr * nq; item += WL_THREADS) {
          const int r = item / nq, q = item - r * nq;
          const WlSpan sp = wl_span(y0 + r, a.H, a.th, a.narrow);
          const uint8_t* src = frame + (long)s0 * 3 + 16 * q;
          uint32_t v[16];
#pragma unroll
          for (int k = 0; k < 16; ++k) v[k] = 0;
          for (int k0 = 0; k0 < sp.nk; k0 += WL_UNROLL) {
            uint32_t w[WL_UNROLL];
            uint4 d[WL_UNROLL];
#pragma unroll
            for (int i = 0; i < WL_UNROLL; ++i) {
              const int k = k0 + i;
              w[i] = k < sp.nk ? wl_weight(k, sp.r, a.H, a.th) : 0u;
              const uint8_t* p = src + (long)min(sp.j0 + k, a.H - 1) * rowb;   // past the footprint: weight 0
              if (VEC) {
                d[i] = *reinterpret_cast<const uint4*>(p);
              } else {
                uint32_t e[4] = {0, 0, 0, 0};
#pragma unroll
                for (int c = 0; c < 16; ++c)
                  if (16 * q + c < snb) e[c >> 2] |= (uint32_t)p[c] << (8 * (c & 3));
                d[i] = make_uint4(e[0], e[1], e[2], e[3]);
              }
            }
#pragma unroll
            for (int i = 0; i < WL_UNROLL; ++i) {
              const uint32_t e[4] = {d[i].x, d[i].y, d[i].z, d[i].w};
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                v[4 * c + 0] += w[i] * (e[c] & 0xffu);
                v[4 * c + 1] += w[i] * ((e[c] >> 8) & 0xffu);
                v[4 * c + 2] += w[i] * ((e[c] >> 16) & 0xffu);
                v[4 * c + 3] += w[i] * (e[c] >> 24);
              }
            }
          }
          uint4* dst = reinterpret_cast<uint4*>(s_v + r * segp + 16 * q);
#pragma unroll
          for (int c = 0; c < 4; ++c) dst[c] = make_uint4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < WL_ACC; ++u) {
          if (irow[u] < 0 || irow[u] >= nr) continue;
          const WlSpan sp = isp[u];
          const int ka = max(0, s0 - sp.j0), kb = min(sp.nk, s0 + sn - sp.j0);
          const uint32_t* col = s_v + irow[u] * segp + (sp.j0 - s0) * 3 + ich[u];
          uint32_t S = 0;
          for (int k = ka; k < kb; ++k) S += wl_weight(k, sp.r, a.W, a.tw) * col[3 * k];
          acc[u] += S;
        }
        __syncthreads();                                              // the image is rewritten by the next segment
      }

#pragma unroll
      for (int u = 0; u < WL_ACC; ++u) {
        if (irow[u] < 0 || irow[u] >= nr) continue;
        const int y = y0 + irow[u], x = xc0 + icol[u], c = ich[u];
        uint32_t val = (2u * acc[u] + WH) / (2u * WH);
        if (ringed && min(min(y, x), min(a.th - 1 - y, a.tw - 1 - x)) < a.ring) val = wl_channel(a.alert, c);
        const int ly = y - a.ring, lx = x - a.ring;
        if (a.ls > 0 && ly >= 0 && ly < boxh && lx >= 0 && lx < boxw) {
          bool ink = false;
          if (ly >= a.ls && lx >= a.ls) {
            const int gy = (ly - a.ls) / a.ls, gx = (lx - a.ls) / a.ls;
            const int d = gx / 6, bit = gx - 6 * d;
            ink = (wl_digits[s_dig[d]][gy] >> (7 - bit)) & 1;
          }
          val = wl_channel(ink ? a.fg : a.lbg, c);
        }
        a.wall[(prow + oy + y) * pitch + (long)(ox + x) * 3 + c] = (uint8_t)val;
      }
    }
  }
}

// One workgroup.  Index order: slot j shows camera j while j < B.  Score order: the cameras with
// score >= min_score by score descending, ties to the lower index; a camera's slot is its rank,
// the number of cameras that come before it, counted against the scores in LDS (B <= WL_SEL_MAX: at
// most 4 cameras per thread, B comparisons each, every lane of a wave reading the same word).
// Ranks are distinct, so no two threads write one slot; slots from the number of eligible cameras
// on are -1.
__global__ __launch_bounds__(WL_SEL_THREADS) void wall_select_kernel(const int* __restrict__ score,
                                                                      int* __restrict__ source, int B, long slots,
                                                                      int by_score, int min_score) {
  __shared__ int s_score[WL_SEL_MAX];
  __shared__ int s_cnt[WL_SEL_THREADS / 64];
  const int tid = threadIdx.x;
  if (!by_score) {
    for (long j = tid; j < slots; j += WL_SEL_THREADS) source[j] = j < B ? (int)j : -1;
    return;
  }
  int mine = 0;
  for (int b = tid; b < B; b += WL_SEL_THREADS) {
    const int v = score[b];
    s_score[b] = v;
    mine += v >= min_score ? 1 : 0;
  }
  for (int s = 32; s >= 1; s >>= 1) mine += __shfl_xor(mine, s);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = mine;
  __syncthreads();
  int M = 0;
#pragma unroll
  for (int w = 0; w < WL_SEL_THREADS / 64; ++w) M += s_cnt[w];
  for (int b = tid; b < B; b += WL_SEL_THREADS) {
    const int v = s_score[b];
    if (v < min_score) continue;
    int rank = 0;
    for (int o = 0; o < B; ++o) {
      const int vo = s_score[o];
      rank += (vo > v || (vo == v && o < b)) ? 1 : 0;
    }
    if (rank < slots) source[rank] = b;
  }
  for (long j = (long)M + tid; j < slots; j += WL_SEL_THREADS) source[j] = -1;
}

}  // namespace aiko

// score int32 [B] (null in index order), source int32 [slots].  order 0 index, 1 score (B <= 4096).
// Returns -1 for a configuration the launch does not cover.
extern "C" int aiko_wall_select(const int* score, int* source, int B, long slots, int order, int min_score,
                                hipStream_t stream) {
  if (B < 1 || slots < 1 || slots > INT32_MAX || order < 0 || order > 1 ||
      (order == 1 && (!score || B > aiko::WL_SEL_MAX)))
    return -1;
  aiko::wall_select_kernel<<<1, aiko::WL_SEL_THREADS, 0, stream>>>(score, source, B, slots, order, min_score);
  return (int)hipGetLastError();
}

// frames uint8 [B, H, W, 3], score int32 [B] or null, source int32 [P * R * C] (a camera or -1; a
// value outside [0, B) is an empty tile), wall uint8 [P, R th + (R + 1) g, C tw + (C + 1) g, 3].
// Colours are R | G << 8 | B << 16.  Returns -1 for a configuration the launch does not cover.
extern "C" int aiko_wall_compose(const void* frames, const int* score, const int* source, void* wall, int B, int H,
                                 int W, int R, int C, int th, int tw, int g, int P, int min_score, int ring,
                                 int label_scale, int label_base, int background, int alert, int label_fg,
                                 int label_bg, hipStream_t stream) {
  const auto colour = [](int c) { return c >= 0 && c <= 0xffffff; };
  if (B < 1 || H < 1 || W < 1 || (long)H * W > (1L << 23) || R < 1 || C < 1 || (long)R * C > 1024 || th < 1 ||
      th > H || tw < 1 || tw > W || g < 0 || g > 64 || P < 1 || ring < 0 || 2 * ring > (th < tw ? th : tw) ||
      label_scale < 0 || label_scale > 4 || label_base < 0 || (long)label_base + B > INT32_MAX ||
      !colour(background) || !colour(alert) || !colour(label_fg) || !colour(label_bg))
    return -1;
  const long Hw = (long)R * th + (long)(R + 1) * g, Ww = (long)C * tw + (long)(C + 1) * g;
  const long slots = (long)P * R * C;
  if (Hw > (1 << 24) || Ww > (1 << 24) || slots >= (1 << 24)) return -1;      // slots x threads < 2^32
  aiko::WallArgs a;
  a.frames = static_cast<const uint8_t*>(frames);
  a.score = score;
  a.source = source;
  a.wall = static_cast<uint8_t*>(wall);
  a.B = B; a.H = H; a.W = W; a.R = R; a.C = C; a.th = th; a.tw = tw; a.g = g;
  a.Hw = (int)Hw; a.Ww = (int)Ww;
  a.min_score = min_score; a.ring = ring; a.ls = label_scale; a.label_base = label_base;
  a.bg = (uint32_t)background; a.alert = (uint32_t)alert; a.fg = (uint32_t)label_fg; a.lbg = (uint32_t)label_bg;
  // a pass: nxc output columns whose source span (plus the 15 pixels a segment may start early)
  // fits one LDS segment where an output column is narrower than that, as many rows as then fit
  const int seg_max = aiko::WL_LDS / 3 / 16 * 16;                     // 2048
  const auto span = [&](long n) { return (n * W + tw - 1) / tw + 17; };
  long nxc = tw < aiko::WL_OUT / 3 ? tw : aiko::WL_OUT / 3;
  if (span(nxc) > seg_max) {
    nxc = (long)(seg_max - 17) * tw / W;
    if (nxc < 1) nxc = 1;
  }
  long seg = (span(nxc) + 15) / 16 * 16;
  if (seg > seg_max) seg = seg_max;
  if (seg > ((long)W + 15) / 16 * 16) seg = ((long)W + 15) / 16 * 16;
  long rows = aiko::WL_OUT / (3 * nxc);
  if (rows > seg_max / seg) rows = seg_max / seg;
  if (rows > th) rows = th;
  if (rows < 1) rows = 1;
  // a band: about 32 source rows, and no more bands than a grid holds
  long band = (32L * th + H - 1) / H;
  if (band < (th + 65534) / 65535) band = (th + 65534) / 65535;
  band = (band + rows - 1) / rows * rows;
  a.nxc = (int)nxc; a.seg = (int)seg; a.rows = (int)rows; a.band = (int)band;
  a.narrow = (uint64_t)th * H <= UINT32_MAX && (uint64_t)tw * W <= UINT32_MAX ? 1 : 0;
  const dim3 grid((unsigned)slots, (unsigned)((th + band - 1) / band));
  const bool vec = W % 16 == 0 && reinterpret_cast<uintptr_t>(frames) % 16 == 0;
  if (vec)
    aiko::wall_compose_kernel<true><<<grid, aiko::WL_THREADS, 0, stream>>>(a);
  else
    aiko::wall_compose_kernel<false><<<grid, aiko::WL_THREADS, 0, stream>>>(a);
  return (int)hipGetLastError();
}

// The wall: wall_select, then wall_compose on what it wrote.  passes: 3, or 1 / 2 for one launch
// alone (measurements; 2 reads a source the caller filled).
extern "C" int aiko_frame_wall(const void* frames, const int* score, int* source, void* wall, int B, int H, int W,
                               int R, int C, int th, int tw, int g, int P, int order, int min_score, int ring,
                               int label_scale, int label_base, int background, int alert, int label_fg,
                               int label_bg, int passes, hipStream_t stream) {
  if (passes < 1 || passes > 3 || R < 1 || C < 1 || P < 1 || (long)R * C > 1024) return -1;
  if (passes & 1) {
    const int rc = aiko_wall_select(score, source, B, (long)P * R * C, order, min_score, stream);
    if (rc) return rc;
  }
  if (passes & 2)
    return aiko_wall_compose(frames, score, source, wall, B, H, W, R, C, th, tw, g, P, min_score, ring, label_scale,
                             label_base, background, alert, label_fg, label_bg, stream);
  return 0;
}
