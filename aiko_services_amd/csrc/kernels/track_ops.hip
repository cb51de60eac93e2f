// Object identity across frames (gfx950): a greedy IoU tracker over the detector's fixed-size NMS
// output (``det`` [B, max_det, 6] + ``count`` [B], detect_ops.hip).  Batch row b is one camera; its
// table of T track slots stays in HBM between frames and one launch advances every row by one
// frame.  Rows, counts and the table are read by the kernel, so tracking is one more
// graph-replayable launch behind the detector: no host copy, no synchronisation.
//
// The rules (ops/track.py states them in full; ops/reference.py track_ref is the same in plain
// loops and equals this kernel bit for bit):
//   * geometry in fp32, every operation rounded on its own; the threshold test and the order of
//     two pairs are exact: products of two fp32 values in fp64;
//   * greedy: the eligible pair of highest IoU whose track and detection are both unmatched
//     matches, ties to the lower track slot, then to the lower detection index; repeat (here:
//     every pair that is the best of both its sides at once, round after round — the same result);
//   * matched tracks take the detection's box, unmatched ones age and die past max_age, then the
//     unmatched detections are born into the lowest free slots in index order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aiko_api.h"

namespace aiko {

constexpr int TR_WAVE = 64;                            // one wave64 per row: lane t owns track slot t,
                                                       // lane i detection i; masks are 64 bits wide

struct TrackArgs {
  const float* det;             // [B, max_det, 6]
  const int* count;             // [B]
  const float4* boxes;          // [B, T] state in
  const int4* meta;             // [B, T] (id, cls, hits, missed)
  const int* issued;            // [B]
  float4* boxes_out;            // state out: another allocation
  int4* meta_out;
  int* issued_out;
  int* ids;                     // [B*K]
  int* hits;
  int* labels;
  int max_det, K, T;
  float thr, min_score;
  int max_age, class_aware, label_mod;
};

// Intersection and union of two boxes, fp32, one rounding per operation.  hipcc would fuse
// aw * ah into the following sum (roi_rect.h), hence plain operators under ``fp contract(off)``.
__device__ __forceinline__ void pair_geometry(const float4 a, const float4 b, float& inter, float& uni) {
#pragma clang fp contract(off)
  const float aw = a.z - a.x, ah = a.w - a.y;
  const float area_a = aw * ah;
  const float bw = b.z - b.x, bh = b.w - b.y;
  const float area_b = bw * bh;
  const float iw = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float ih = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  inter = iw * ih;
  uni = (area_a + area_b) - inter;
}

// IoU of p above IoU of q, exactly: the cross products of fp32 values are exact in fp64.
__device__ __forceinline__ bool iou_above(float ip, float up, float iq, float uq) {
#pragma clang fp contract(off)
  return (double)ip * (double)uq > (double)iq * (double)up;
}

__device__ __forceinline__ int wrap_inc(int v) { return (int)((unsigned)v + 1u); }

// Grid B, one wave per row.  Every loop runs over the bits of a mask of detections (at most K) or
// of tracks (at most T), or over rounds that each match at least one track (at most T), whatever
// the state holds; a NaN anywhere in a pair fails its comparisons, which leaves the pair ineligible.
__global__ __launch_bounds__(TR_WAVE) void track_detections_kernel(const TrackArgs a) {
  __shared__ float4 s_box[TR_WAVE];                   // the row's detections
  __shared__ int s_cls[TR_WAVE];
  __shared__ int s_id[TR_WAVE], s_hits[TR_WAVE];      // per detection: the track it ended in
  __shared__ float4 s_tbox[TR_WAVE];                  // the row's tracks, for the detections' side
  __shared__ int s_bd[TR_WAVE], s_bt[TR_WAVE];        // a round's best detection per track, best track per detection

  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = min(max(a.count[b], 0), a.K);         // rows read; the rest never is

  // detection `lane`
  float4 dbox = make_float4(0.f, 0.f, 0.f, 0.f);
  float dscore = 0.f;
  int dcls = 0;
  bool dvalid = false;
  if (lane < n) {
    const float* row = a.det + ((long)b * a.max_det + lane) * 6;
    dbox = make_float4(row[0], row[1], row[2], row[3]);
    dscore = row[4];
    dcls = (int)row[5];                               // NaN -> 0, saturating: the class draw_detections shows
    dvalid = isfinite(dbox.x) && isfinite(dbox.y) && isfinite(dbox.z) && isfinite(dbox.w);
  }
  s_box[lane] = dbox;
  s_cls[lane] = dcls;
  s_id[lane] = 0;
  s_hits[lane] = 0;
  const unsigned long long valid = __ballot(dvalid);

  // track slot `lane`
  float4 tbox = make_float4(0.f, 0.f, 0.f, 0.f);
  int4 tm = make_int4(0, 0, 0, 0);
  if (lane < a.T) {
    tbox = a.boxes[(long)b * a.T + lane];
    tm = a.meta[(long)b * a.T + lane];
  }
  s_tbox[lane] = tbox;
  const bool live = lane < a.T && tm.x != 0;
  const int issued = a.issued[b];
  __syncthreads();

  // the detections this track may take, and the best of them: the lowest index among those of
  // highest IoU
  unsigned long long elig = 0ull;
  int best_d = -1;
  float best_i = 0.f, best_u = 1.f;
  auto scan_track = [&](unsigned long long m, bool test) {
    best_d = -1;
    for (; m; m &= m - 1ull) {
      const int d = __ffsll((long long)m) - 1;
      float inter, uni;
      pair_geometry(tbox, s_box[d], inter, uni);
      if (test) {
        const bool cls_ok = !a.class_aware || s_cls[d] == tm.y;
        if (!(cls_ok && inter > 0.f && uni > 0.f && (double)inter >= (double)a.thr * (double)uni)) continue;
        elig |= 1ull << d;
      }
      if (best_d < 0 || iou_above(inter, uni, best_i, best_u)) {
        best_d = d;
        best_i = inter;
        best_u = uni;
      }
    }
  };
  if (live) scan_track(valid, true);

  // the same from the detection's side: the tracks that may take detection `lane` (the transpose
  // of elig, a ballot per detection) and the best of them, the lowest slot among those of highest IoU
  unsigned long long elig_t = 0ull;
  for (unsigned long long m = valid; m; m &= m - 1ull) {          // uniform
    const int d = __ffsll((long long)m) - 1;
    const unsigned long long col = __ballot((elig >> d) & 1ull);
    if (lane == d) elig_t = col;
  }
  int best_t = -1;
  float dbest_i = 0.f, dbest_u = 1.f;
  auto scan_det = [&](unsigned long long m) {
    best_t = -1;
    for (; m; m &= m - 1ull) {
      const int t = __ffsll((long long)m) - 1;
      float inter, uni;
      pair_geometry(s_tbox[t], dbox, inter, uni);
      if (best_t < 0 || iou_above(inter, uni, dbest_i, dbest_u)) {
        best_t = t;
        dbest_i = inter;
        dbest_u = uni;
      }
    }
  };
  scan_det(elig_t);

  // Rounds: a pair matches when each side is the other's best among what is still free.  Under
  // the strict order of pairs (IoU, then slot, then index) no pair that shares its track or its
  // detection comes before such a pair, so the greedy walk matches it too, and what is left after
  // taking all of them out is again a greedy problem.  The first pair of the remaining order is
  // always one of them: every round matches at least one track.
  unsigned long long free_det = valid, free_trk = __ballot(live);   // wave-uniform
  int match = -1;                                     // the detection this track took
  for (int round = 0; round < a.T; ++round) {
    s_bd[lane] = best_d;
    s_bt[lane] = best_t;
    __syncthreads();
    const bool t_won = best_d >= 0 && s_bt[best_d] == lane;
    const bool d_won = best_t >= 0 && s_bd[best_t] == lane;
    __syncthreads();                                  // the next round rewrites both
    const unsigned long long mt = __ballot(t_won), md = __ballot(d_won);
    if (!mt) break;                                   // uniform: no eligible pair is left
    free_trk &= ~mt;
    free_det &= ~md;
    if (t_won) {
      match = best_d;
      best_d = -1;
    } else if (best_d >= 0 && !((free_det >> best_d) & 1ull)) {
      scan_track(elig & free_det, false);
    }
    if (d_won)
      best_t = -1;
    else if (best_t >= 0 && !((free_trk >> best_t) & 1ull))
      scan_det(elig_t & free_trk);
  }

  // matched: the detection's box; unmatched: one frame older, freed past max_age
  int4 om = make_int4(0, 0, 0, 0);
  float4 ob = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    if (match >= 0) {
      ob = s_box[match];
      om = make_int4(tm.x, a.class_aware ? tm.y : s_cls[match], wrap_inc(tm.z), 0);
    } else {
      const int missed = wrap_inc(tm.w);
      if (!(missed > a.max_age)) {
        ob = tbox;
        om = make_int4(tm.x, tm.y, tm.z, missed);
      }
    }
  }

  // births: the j-th free slot takes the j-th unmatched detection that scores enough
  const unsigned long long born = __ballot(dvalid && ((free_det >> lane) & 1ull) && dscore >= a.min_score);
  const unsigned long long free_slots = __ballot(lane < a.T && om.x == 0);
  const int births = min(__popcll(born), __popcll(free_slots));
  if (lane < a.T && om.x == 0) {
    const int j = __popcll(free_slots & ((1ull << lane) - 1ull));
    if (j < births) {
      unsigned long long m = born;
      for (int i = 0; i < j; ++i) m &= m - 1ull;      // j < popcount(born) <= K
      const int d = __ffsll((long long)m) - 1;
      match = d;
      ob = s_box[d];
      om = make_int4((int)((unsigned)issued + (unsigned)j + 1u), s_cls[d], 1, 0);
    }
  }
  if (lane < a.T) {
    a.boxes_out[(long)b * a.T + lane] = ob;
    a.meta_out[(long)b * a.T + lane] = om;
    if (match >= 0) {                                 // matched or born: one track per detection
      s_id[match] = om.x;
      s_hits[match] = om.z;
    }
  }
  if (lane == 0) a.issued_out[b] = (int)((unsigned)issued + (unsigned)births);
  __syncthreads();

  if (lane < a.K) {
    const int id = s_id[lane];
    const long slot = (long)b * a.K + lane;
    a.ids[slot] = id;
    a.hits[slot] = s_hits[lane];
    a.labels[slot] = id > 0 ? id % a.label_mod : -1;
  }
}

}  // namespace aiko

// det fp32 [B, max_det, 6], count int32 [B]; state boxes fp32 [B, T, 4], meta int32 [B, T, 4],
// issued int32 [B], in and out (16-byte aligned boxes and meta, out no alias of in); ids / hits /
// labels int32 [B*K].  Returns -1 for a configuration the launch does not cover.
extern "C" int aiko_track_detections(const float* det, const int* count, const float* boxes, const int* meta,
                                     const int* issued, float* boxes_out, int* meta_out, int* issued_out, int* ids,
                                     int* hits, int* labels, int B, int max_det, int K, int T, float thr, int max_age,
                                     float min_score, int class_aware, int label_mod, hipStream_t stream) {
  if (B < 1 || B > 65535 || K < 1 || K > aiko::TR_WAVE || K > max_det || T < 1 || T > aiko::TR_WAVE ||
      !(thr > 0.f) || !(thr <= 1.f) || max_age < 0 || label_mod < 1)
    return -1;
  aiko::TrackArgs a;
  a.det = det;
  a.count = count;
  a.boxes = reinterpret_cast<const float4*>(boxes);
  a.meta = reinterpret_cast<const int4*>(meta);
  a.issued = issued;
  a.boxes_out = reinterpret_cast<float4*>(boxes_out);
  a.meta_out = reinterpret_cast<int4*>(meta_out);
  a.issued_out = issued_out;
  a.ids = ids;
  a.hits = hits;
  a.labels = labels;
  a.max_det = max_det; a.K = K; a.T = T;
  a.thr = thr; a.min_score = min_score;
  a.max_age = max_age; a.class_aware = class_aware ? 1 : 0; a.label_mod = label_mod;
  aiko::track_detections_kernel<<<dim3((unsigned)B), aiko::TR_WAVE, 0, stream>>>(a);
  return (int)hipGetLastError();
}
