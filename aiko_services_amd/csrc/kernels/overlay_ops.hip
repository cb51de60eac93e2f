// Detection overlay (gfx950): boxes and labels of the detector's fixed-size NMS output (``det``
// [B, max_det, 6] + ``count`` [B], detect_ops.hip; optionally a classifier's per-slot class and
// probability) drawn into uint8 frames on the device.  Rows and counts are read by the kernel, so
// the annotated frames are one more graph-replayable launch behind roi_crop and the classifier.
//
// Every output pixel is a function of the same input pixel and the frame's rows only, which makes
// drawing in place (out == frames) safe.  All arithmetic is integer except the rect (roi_rect.h,
// the rect of roi_crop) and the two-digit percentage (one fp32 multiply, round half to even).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "roi_rect.h"
#include "aiko_api.h"

namespace aiko {

constexpr int OV_TW = 128, OV_TH = 32;               // pixels per tile: one workgroup
constexpr int OV_THREADS = 256;
constexpr int OV_TPR = OV_TW / 4;                     // threads per tile row, 4 adjacent pixels each
constexpr int OV_WROWS = OV_TH / (OV_THREADS / 64);   // consecutive tile rows owned by one wave
constexpr int OV_PSTEP = 64 / OV_TPR;                 // rows a wave covers per pass
constexpr int OV_PASSES = OV_WROWS / OV_PSTEP;        // passes: rows py, py + OV_PSTEP, ...
constexpr int OV_CHUNK = OV_THREADS;                  // detection rows culled per round, one per thread
constexpr int OV_TEXT = 36;                            // characters kept per label: 32 + space + two digits
constexpr int OV_FONT_LDS = 2048;                     // atlas bytes staged in LDS (a larger one is read in place)
constexpr uint32_t OV_ALL = 0xffffu;                  // one bit per pixel of a thread
static_assert(OV_PASSES * 4 == 16 && OV_THREADS == 256, "done mask and wave count below");

struct OverlayArgs {
  const uint8_t* frames;
  uint8_t* out;
  const float* det;
  const int* count;
  const int* labels;            // [B*K] or null: the class is (int)det[b, i, 5]
  const float* scores;          // [B*K] or null: the score is det[b, i, 4]
  const uint8_t* names;         // [C, L] zero-padded ASCII
  const uint8_t* font;          // [G, gh], bit 7 = leftmost pixel, glyph g = code 32 + g
  const uint8_t* palette;       // [P, 3]
  int H, W, max_det, K, C, L, G, gh, P;
  int cw, ch;                   // character cell in pixels: gw * s, gh * s
  int t, s;
  float margin;
  int show_score, in_place;
};

// One pixel of the label of a culled row, (u, v) its position inside the text area.  ``text`` is
// the row's characters in LDS, ``font`` the atlas (staged in LDS when it fits); colw = the row's
// colour | (white text) << 24.  u / cw, v / s and (u % cw) / s are taken as (n + 0.5) * (1 / d)
// in fp32, truncated: exact for n < 2^11, d <= 32 (the error of the product stays below the
// 0.5 / d that separates it from the next integer).
__device__ __forceinline__ uint32_t label_pixel(const OverlayArgs& a, int u, int v, int nch, const uint8_t* text,
                                                const uint8_t* font, float inv_cw, float inv_s, uint32_t colw) {
  uint32_t px = colw & 0xffffffu;
  if (u >= 0 && u < nch * a.cw && v >= 0 && v < a.ch) {
    const int j = (int)(((float)u + 0.5f) * inv_cw);
    const int g = (int)text[j] - 32;
    if (g >= 0 && g < a.G) {
      const uint32_t bits = font[g * a.gh + (int)(((float)v + 0.5f) * inv_s)];
      const int col = (int)(((float)(u - j * a.cw) + 0.5f) * inv_s);
      if ((bits >> (7 - col)) & 1u) px = (colw >> 24) & 1u ? 0xffffffu : 0u;
    }
  }
  return px;
}

// Bits k = 0..3 set iff a <= px + k < b.
__device__ __forceinline__ uint32_t range4(int a, int b, int px) {
  const int lo = min(max(a - px, 0), 4), hi = min(max(b - px, 0), 4);
  return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// Grid (tiles x, tiles y, B), one OV_TW x OV_TH tile per workgroup.  Per round of OV_CHUNK rows:
// every thread takes one used row of the frame, computes its rect and label once and keeps it iff
// its outline or label touches the tile (a tile wholly inside a box's interior and off its label
// needs no entry); a wave ballot compacts the kept rows — rect, label rect, colour and the label's
// characters — into LDS in index order.  The pixels then walk that list and stop at the first
// hit: the lowest row index wins, the label before the outline.  A thread owns 4 adjacent pixels
// in each of OV_PASSES rows and tests a list entry as one 16-bit mask (4 column bits, a row test per
// pass), since the walk is what costs at long lists (profiles/overlay.md).  A tile whose lists are
// all empty is a plain copy (nothing at all when in place).  Out
// of place the pixels are loaded before the cull, so its chain of dependent loads (count, row,
// class, name) overlaps with theirs.
// VEC: W % 4 == 0 and both tensors 4-byte aligned, so a thread's 4 pixels are three aligned dwords.
template <bool VEC>
__global__ __launch_bounds__(OV_THREADS) void draw_detections_kernel(const OverlayArgs a) {
  __shared__ int4 s_rect[OV_CHUNK];                   // X0, Y0, X1, Y1
  __shared__ int4 s_lab[OV_CHUNK];                    // lx, ly, clipped end x, clipped end y
  __shared__ uint32_t s_col[OV_CHUNK];
  __shared__ int s_nch[OV_CHUNK];                     // characters of the label
  __shared__ __attribute__((aligned(4))) uint8_t s_text[OV_CHUNK][OV_TEXT];   // the label's characters
  __shared__ uint8_t s_font[OV_FONT_LDS];             // the atlas, when it fits
  __shared__ int s_wcnt[OV_THREADS / 64], s_wlab[OV_THREADS / 64];

  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * OV_TW, ty0 = blockIdx.y * OV_TH;
  const int tx1 = min(tx0 + OV_TW, a.W), ty1 = min(ty0 + OV_TH, a.H);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // a wave owns a strip of OV_WROWS consecutive tile rows (two per pass), so a row that misses
  // the strip is skipped by the whole wave
  const int px = tx0 + (tid % OV_TPR) * 4;            // the first of this thread's 4 pixels
  const int sy0 = ty0 + wave * OV_WROWS;              // the wave's strip
  const int py = sy0 + lane / OV_TPR;                 // this thread's row in pass 0; pass p adds p * OV_PSTEP
  const long frame = (long)b * a.H;

  uint32_t pix[OV_PASSES][4];                         // RGB in the low 24 bits
  uint32_t oob = 0;                                   // pixels outside the frame
#pragma unroll
  for (int p = 0; p < OV_PASSES; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pix[p][i] = 0;
      if (py + p * OV_PSTEP >= ty1 || px + i >= tx1) oob |= 1u << (4 * p + i);
    }
  uint32_t done = oob;
  bool loaded = false, font_ready = false;            // workgroup-uniform

  auto load = [&]() {
#pragma unroll
    for (int p = 0; p < OV_PASSES; ++p) {
      const int y = py + p * OV_PSTEP;
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

  if (!a.in_place) {                                  // needed whatever the rows say: in flight during the cull
    load();
    loaded = true;
  }
  const int n = min(max(a.count[b], 0), a.K);         // used rows of this frame
  const bool staged = a.G * a.gh <= OV_FONT_LDS;
  const uint8_t* font = staged ? s_font : a.font;
  const float inv_cw = 1.0f / (float)a.cw, inv_s = 1.0f / (float)a.s;
  const int Lh = a.ch + 2 * a.s;
  const int Lw_max = (a.L + 3) * a.cw + 2 * a.s;      // the widest label: name, space, two digits

  for (int c0 = 0; c0 < n; c0 += OV_CHUNK) {
    const int i = c0 + tid;
    bool keep = false, lab_hit = false;
    RoiRect r{0, 0, 0, 0};
    int4 lab = make_int4(0, 0, 0, 0);
    uint32_t colw = 0;
    int nlen = 0, nch = 0, pct = 0;
    uint32_t nm[8] = {0, 0, 0, 0, 0, 0, 0, 0};        // the name's bytes, packed: constant indices only
    if (i < n) {
      const float* row = a.det + ((long)b * a.max_det + i) * 6;
      const float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
      if (isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2)) {
        r = roi_rect(x1, y1, x2, y2, a.margin, a.H, a.W);
        // bounds that hold for any text: the label lies in rows [Y0 - Lh, Y0 + Lh) and in columns
        // [X0 - Lw_max, X0 + Lw_max); most rows are dropped here without reading class or name
        if (max(r.y0 - Lh, 0) < ty1 && max(r.y1, r.y0 + Lh) > ty0 && max(r.x0 - Lw_max, 0) < tx1 &&
            max(r.x1, r.x0 + Lw_max) > tx0) {
          const long slot = (long)b * a.K + i;
          const int cls = a.labels ? a.labels[slot] : (int)row[5];
          const float prob = a.scores ? a.scores[slot] : row[4];
          if (cls >= 0 && cls < a.C) {
            const uint8_t* src = a.names + (long)cls * a.L;
            nlen = a.L;
#pragma unroll
            for (int j = 31; j >= 0; --j) {           // independent loads: one round trip, not L
              const uint32_t c = j < a.L ? src[j] : 1u;
              nm[j >> 2] |= c << (8 * (j & 3));
              if (c == 0) nlen = j;
            }
          }
          nch = nlen + (a.show_score ? (nlen ? 3 : 2) : 0);
          pct = (int)fminf(fmaxf(rintf(prob * 100.0f), 0.f), 99.f);             // NaN -> 0
          const uint8_t* pc = a.palette + (cls >= 0 ? cls % a.P : 0) * 3;
          const uint32_t R = pc[0], G = pc[1], Bl = pc[2];
          const uint32_t white = 299u * R + 587u * G + 114u * Bl >= 128000u ? 0u : 1u;
          colw = R | (G << 8) | (Bl << 16) | (white << 24);
          lab = make_int4(r.x0, r.y0, r.x0, r.y0);    // no characters: an empty label
          if (nch > 0) {
            const int Lw = nch * a.cw + 2 * a.s;
            const int lx = max(min(r.x0, a.W - Lw), 0);
            const int ly = r.y0 - Lh >= 0 ? r.y0 - Lh : r.y0;
            lab = make_int4(lx, ly, min(lx + Lw, a.W), min(ly + Lh, a.H));
            lab_hit = lab.x < tx1 && lab.z > tx0 && lab.y < ty1 && lab.w > ty0;
          }
          const bool rect_hit = r.x0 < tx1 && r.x1 > tx0 && r.y0 < ty1 && r.y1 > ty0;
          const bool interior = tx0 >= r.x0 + a.t && tx1 <= r.x1 - a.t && ty0 >= r.y0 + a.t && ty1 <= r.y1 - a.t;
          keep = lab_hit || (rect_hit && !interior);
        }
      }
    }
    // compaction in index order: wave w holds rows c0 + 64 w ..., a lane's place is the number of
    // kept rows in front of it
    const unsigned long long m = __ballot(keep);
    const unsigned long long ml = __ballot(keep && lab_hit);
    if (lane == 0) {
      s_wcnt[wave] = __popcll(m);
      s_wlab[wave] = ml != 0ull;
    }
    __syncthreads();
    int base = 0, total = 0, labels = 0;              // labels: some kept row has label pixels in this tile
#pragma unroll
    for (int w = 0; w < OV_THREADS / 64; ++w) {
      const int c = s_wcnt[w];
      base += w < wave ? c : 0;
      total += c;
      labels += s_wlab[w];
    }
    if (keep) {
      const int e = base + __popcll(m & ((1ull << lane) - 1ull));
      s_rect[e] = make_int4(r.x0, r.y0, r.x1, r.y1);
      s_lab[e] = lab;
      s_col[e] = colw;
      s_nch[e] = nch;
      uint32_t* text = reinterpret_cast<uint32_t*>(s_text[e]);     // rows of OV_TEXT bytes: 4-byte aligned
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (4 * j < nlen) text[j] = nm[j];            // bytes past the name are overwritten or never read
      if (nch > nlen) {                               // [space] digit digit
        if (nlen) s_text[e][nlen] = 32;
        s_text[e][nch - 2] = (uint8_t)(48 + pct / 10);
        s_text[e][nch - 1] = (uint8_t)(48 + pct % 10);
      }
    }
    __syncthreads();

    if (total > 0) {
      if (!loaded) {
        load();
        loaded = true;
      }
      if (labels && staged && !font_ready) {          // workgroup-uniform: the atlas only where text is drawn
        for (int j = tid; j < a.G * a.gh; j += OV_THREADS) s_font[j] = a.font[j];
        __syncthreads();
        font_ready = true;
      }
      for (int e = 0; e < total && done != OV_ALL; ++e) {
        const int4 rc = s_rect[e], lb = s_lab[e];
        const uint32_t cw_ = s_col[e];
        const int uy0 = min(rc.y, lb.y), uy1 = max(rc.w, lb.w);
        if (uy0 >= sy0 + OV_WROWS || uy1 <= sy0) continue;             // misses the wave's strip
        if (px + 4 <= min(rc.x, lb.x) || px >= max(rc.z, lb.z)) continue;   // ... or this thread's columns
        // the row's hits as bit masks: the 4 columns once, then one nibble per pass
        const uint32_t mx_rect = range4(rc.x, rc.z, px);
        const uint32_t mx_edge = mx_rect & ~range4(rc.x + a.t, rc.z - a.t, px);
        const uint32_t mx_lab = range4(lb.x, lb.z, px);
        uint32_t lab16 = 0, out16 = 0;
#pragma unroll
        for (int p = 0; p < OV_PASSES; ++p) {
          const int y = py + p * OV_PSTEP;
          const bool yrect = y >= rc.y && y < rc.w;
          const bool yedge = y < rc.y + a.t || y >= rc.w - a.t;
          const bool ylab = y >= lb.y && y < lb.w;
          out16 |= (yrect ? (yedge ? mx_rect : mx_edge) : 0u) << (4 * p);
          lab16 |= (ylab ? mx_lab : 0u) << (4 * p);
        }
        lab16 &= ~done;                               // an earlier row keeps its pixels,
        out16 &= ~done & ~lab16;                      // and the label covers its own outline
        done |= lab16 | out16;
        if (out16) {
          const uint32_t c = cw_ & 0xffffffu;
#pragma unroll
          for (int p = 0; p < OV_PASSES; ++p)
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if ((out16 >> (4 * p + k)) & 1u) pix[p][k] = c;
        }
        if (lab16) {
          const int nch = s_nch[e];
#pragma unroll
          for (int p = 0; p < OV_PASSES; ++p)
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if ((lab16 >> (4 * p + k)) & 1u)
                pix[p][k] = label_pixel(a, px + k - lb.x - a.s, py + p * OV_PSTEP - lb.y - a.s, nch, s_text[e], font,
                                        inv_cw, inv_s, cw_);
        }
      }
    }
    __syncthreads();                                  // the list is rewritten by the next round
  }

  if (!loaded) return;                                // in place and nothing drawn in this tile
  const uint32_t hit = done & ~oob;
#pragma unroll
  for (int p = 0; p < OV_PASSES; ++p) {
    const int y = py + p * OV_PSTEP;
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

// frames / out uint8 [B, H, W, 3] (out == frames draws in place), det fp32 [B, max_det, 6], count
// int32 [B], labels int32 / scores fp32 [B*K] or null, names uint8 [C, L], font uint8 [G, gh],
// palette uint8 [P, 3].  Returns -1 for a configuration the launch does not cover.
extern "C" int aiko_draw_detections(const void* frames, void* out, const float* det, const int* count,
                                    const int* labels, const float* scores, const void* names, const void* font,
                                    const void* palette, int B, int H, int W, int max_det, int K, int C, int L,
                                    int G, int gh, int gw, int P, int t, int s, float margin, int show_score,
                                    hipStream_t stream) {
  if (B < 1 || H < 1 || W < 1 || K < 1 || K > max_det || C < 0 || L < 1 || L > 32 || G < 0 || gh < 1 || gh > 16 ||
      gw < 1 || gw > 8 || P < 1 || t < 1 || t > 16 || s < 1 || s > 4 || !(margin >= 0.f) || !(margin <= 3.0e38f))
    return -1;
  const long tiles_x = (W + aiko::OV_TW - 1) / aiko::OV_TW, tiles_y = (H + aiko::OV_TH - 1) / aiko::OV_TH;
  if (B > 65535 || tiles_y > 65535 || W > (1 << 24) || H > (1 << 24)) return -1;
  aiko::OverlayArgs a;
  a.frames = static_cast<const uint8_t*>(frames);
  a.out = static_cast<uint8_t*>(out);
  a.det = det;
  a.count = count;
  a.labels = labels;
  a.scores = scores;
  a.names = static_cast<const uint8_t*>(names);
  a.font = static_cast<const uint8_t*>(font);
  a.palette = static_cast<const uint8_t*>(palette);
  a.H = H; a.W = W; a.max_det = max_det; a.K = K; a.C = C; a.L = L; a.G = G; a.gh = gh; a.P = P;
  a.cw = gw * s; a.ch = gh * s; a.t = t; a.s = s;
  a.margin = margin;
  a.show_score = show_score ? 1 : 0;
  a.in_place = frames == out ? 1 : 0;
  const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)B);
  const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(frames) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
  if (vec)
    aiko::draw_detections_kernel<true><<<grid, aiko::OV_THREADS, 0, stream>>>(a);
  else
    aiko::draw_detections_kernel<false><<<grid, aiko::OV_THREADS, 0, stream>>>(a);
  return (int)hipGetLastError();
}
