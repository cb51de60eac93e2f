// torch.ops.aiko.*: the detect head's tail and what works on its detections (decode, NMS, crop,
// warp, draw, redact, track), motion and marker detection, which write detector rows, and the
// camera wall, which is ordered by their counts.
// Each operator validates shapes / dtypes / devices on the host (checks.h holds the shared
// checks) and launches on the caller's current HIP stream.
#include "checks.h"

#include <ATen/ops/empty.h>

namespace {

// feats: per level [B, H, W, 4*reg_max + nc] bf16 (channel slices allowed), strides per level
void yolo_decode_out(at::TensorList feats, at::IntArrayRef strides, int64_t nc, int64_t reg_max,
                     at::Tensor& boxes, at::Tensor& scores, at::Tensor& cls) {
  const int nlev = (int)feats.size();
  TORCH_CHECK(nlev >= 1 && nlev <= 4 && (int)strides.size() == nlev, "aiko.yolo_decode_out: 1..4 levels");
  TORCH_CHECK(reg_max == 16 && nc % 8 == 0, "aiko.yolo_decode_out: reg_max 16, nc % 8 == 0");
  const void* ptrs[4] = {nullptr, nullptr, nullptr, nullptr};
  int H[4] = {0, 0, 0, 0}, W[4] = {1, 1, 1, 1}, st[4] = {1, 1, 1, 1}, ld[4] = {0, 0, 0, 0};
  const int64_t B = feats[0].size(0);
  int64_t A = 0;
  for (int i = 0; i < nlev; ++i) {
    check_cuda(feats[i], "feat");
    ld[i] = (int)pixel_pitch(feats[i], "yolo_decode_out");
    TORCH_CHECK(feats[i].size(0) == B && feats[i].size(3) == 4 * reg_max + nc,
                "aiko.yolo_decode_out: level channels must be 4*reg_max + nc");
    ptrs[i] = feats[i].data_ptr();
    H[i] = feats[i].size(1); W[i] = feats[i].size(2); st[i] = strides[i];
    A += H[i] * W[i];
  }
  check_cuda_all({&boxes, &scores, &cls}, {"boxes", "scores", "cls"});
  TORCH_CHECK(boxes.scalar_type() == at::kFloat && boxes.is_contiguous() && boxes.numel() == B * A * 4 &&
                  scores.scalar_type() == at::kFloat && scores.is_contiguous() && scores.numel() == B * A &&
                  cls.scalar_type() == at::kInt && cls.is_contiguous() && cls.numel() == B * A,
              "aiko.yolo_decode_out: outputs boxes fp32 [B, A, 4], scores fp32 [B, A], cls int32 [B, A]");
  check_launch(aiko_yolo_decode(ptrs, H, W, st, ld, nlev, B, nc, reg_max, boxes.data_ptr(),
                                scores.data_ptr<float>(), cls.data_ptr<int>(), cur_stream()),
               "yolo_decode");
}

// params = [conf, iou, max_wh, gain, pad_l, pad_t, img_w, img_h]
void topk_nms_out(const at::Tensor& boxes, const at::Tensor& scores, const at::Tensor& cls,
                  int64_t max_cand, at::ArrayRef<double> params, at::Tensor& det, at::Tensor& count) {
  check_cuda_all({&boxes, &scores, &cls, &det, &count}, {"boxes", "scores", "cls", "det", "count"});
  TORCH_CHECK(params.size() == 8, "aiko.topk_nms_out: params = [conf, iou, max_wh, gain, pad_l, pad_t, img_w, img_h]");
  // the selection keys are the scores' fp32 bits, ordered like the scores only from +0 up: with
  // conf < 0 a score of 0.0 would get key 0 ("no candidate") and negative scores the largest keys
  TORCH_CHECK(params[0] >= 0.0 && params[1] == params[1],
              "aiko.topk_nms_out: conf must be >= 0 and neither conf nor iou NaN");
  TORCH_CHECK(scores.scalar_type() == at::kFloat && scores.dim() == 2 && scores.is_contiguous(),
              "aiko.topk_nms_out: scores fp32 [B, A]");
  const int64_t B = scores.size(0), A = scores.size(1);
  TORCH_CHECK(A <= 32768, "aiko.topk_nms_out: at most 32768 anchors per image");
  TORCH_CHECK(boxes.scalar_type() == at::kFloat && boxes.is_contiguous() && boxes.numel() == B * A * 4,
              "aiko.topk_nms_out: boxes fp32 [B, A, 4]");
  TORCH_CHECK(cls.scalar_type() == at::kInt && cls.is_contiguous() && cls.numel() == B * A,
              "aiko.topk_nms_out: cls int32 [B, A]");
  const int64_t max_det = check_det(det, B, "topk_nms_out");
  TORCH_CHECK(max_cand >= 1 && max_cand <= 1024 && max_det >= 1 && max_det <= 1024,
              "aiko.topk_nms_out: 1 <= max_candidates, max_det <= 1024");
  TORCH_CHECK(count.scalar_type() == at::kInt && count.numel() == B && count.is_contiguous(),
              "aiko.topk_nms_out: count int32 [B]");
  // G > 1 workgroups per image: mask-block workspace + zeroed counters from the caching
  // allocator (graph-capture safe: the memset is a node of the captured graph)
  const size_t wsb = aiko_topk_nms_workspace((int)B);
  at::Tensor ws;
  if (wsb) {
    ws = at::empty({(int64_t)wsb}, scores.options().dtype(at::kByte));
    ws.narrow(0, (int64_t)wsb - 4 * B, 4 * B).zero_();
  }
  check_launch(aiko_topk_nms(boxes.data_ptr(), scores.data_ptr<float>(), cls.data_ptr<int>(), B, A,
                             max_cand, max_det, params[0], params[1], params[2], params[3], params[4],
                             params[5], params[6], params[7], det.data_ptr<float>(),
                             count.data_ptr<int>(), wsb ? ws.data_ptr() : nullptr, cur_stream()),
               "topk_nms");
}

// crops[b*k + i] <- the rect of det[b, i] (i < min(count[b], k), coordinates finite) resized to
// crops' [Ho, Wo]; rois[b*k + i] <- that rect (x0, y0, x1, y1), half-open; other slots zero
void roi_crop_out(const at::Tensor& frames, const at::Tensor& det, const at::Tensor& count, int64_t k,
                  double margin, at::Tensor& crops, at::Tensor& rois) {
  check_cuda_all({&frames, &det, &count, &crops, &rois}, {"frames", "det", "count", "crops", "rois"});
  check_frames_u8(frames, "roi_crop_out");
  TORCH_CHECK(frames.numel() >= 4, "aiko.roi_crop_out: frames uint8 [B, H, W, 3] contiguous required");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  const int64_t max_det = check_det_count(det, count, B, "roi_crop_out");
  check_k(k, max_det, "roi_crop_out");
  TORCH_CHECK(margin >= 0.0 && margin <= 3.0e38, "aiko.roi_crop_out: a finite margin >= 0 required");
  TORCH_CHECK(B * k <= 65535, "aiko.roi_crop_out: B * k = ", B * k, " ROI slots exceed the grid limit (65535)");
  TORCH_CHECK(crops.scalar_type() == at::kByte && crops.dim() == 4 && crops.size(0) == B * k && crops.size(3) == 3 &&
                  crops.is_contiguous(),
              "aiko.roi_crop_out: crops uint8 [B*k, Ho, Wo, 3] contiguous required");
  const int64_t Ho = crops.size(1), Wo = crops.size(2);
  TORCH_CHECK(Ho >= 1 && Wo >= 4 && Wo % 4 == 0, "aiko.roi_crop_out: crop width must be a multiple of 4, got ", Wo);
  TORCH_CHECK(Ho <= 16384 && Wo <= 16384 && H <= (1 << 24) && W <= (1 << 24),
              "aiko.roi_crop_out: crop side <= 16384, frame side <= 2^24");
  TORCH_CHECK(rois.scalar_type() == at::kInt && rois.dim() == 2 && rois.size(0) == B * k && rois.size(1) == 4 &&
                  rois.is_contiguous(),
              "aiko.roi_crop_out: rois int32 [B*k, 4] contiguous required");
  TORCH_CHECK(aligned(crops, 4) && aligned(rois, 16), "aiko.roi_crop_out: crops 4-byte, rois 16-byte aligned");
  check_launch(aiko_roi_crop_u8(frames.data_ptr(), det.data_ptr<float>(), count.data_ptr<int>(), crops.data_ptr(),
                                rois.data_ptr<int>(), B, H, W, max_det, k, Ho, Wo, (float)margin, cur_stream()),
               "roi_crop_u8");
}

// patches[b*k + i] <- the quad quads[b, i] (i < min(count[b], k), coordinates in -4096..8191, not
// degenerate) of frame b rectified to patches' [Ho, Wo] (warp_ops.hip; the rule is in ops/warp.py);
// valid[b*k + i] <- 1 for such a slot; other slots zero in both.  margin: sixteenths of the side added
// all round; origin 1: the coordinates are pixel centres, 0: pixel edges
void quad_warp_out(const at::Tensor& frames, const at::Tensor& quads, const at::Tensor& count, int64_t k,
                   int64_t margin, int64_t origin, at::Tensor& patches, at::Tensor& valid) {
  const at::Tensor* ins[3] = {&frames, &quads, &count};
  const char* in_names[3] = {"frames", "quads", "count"};
  const at::Tensor* outs[2] = {&patches, &valid};
  const char* out_names[2] = {"patches", "valid"};
  check_cuda_all(ins, in_names);
  check_cuda_all(outs, out_names);
  check_same_device(ins, outs, "quad_warp_out");
  check_frames_u8(frames, "quad_warp_out");
  TORCH_CHECK(frames.numel() >= 4, "aiko.quad_warp_out: frames uint8 [B, H, W, 3] contiguous required");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  TORCH_CHECK(H <= 4096 && W <= 4096, "aiko.quad_warp_out: H = ", H, ", W = ", W,
              " exceed the frame limit (4096 pixels a side)");
  TORCH_CHECK(quads.scalar_type() == at::kInt && quads.dim() == 4 && quads.size(0) == B && quads.size(1) >= 1 &&
                  quads.size(2) == 4 && quads.size(3) == 2 && quads.is_contiguous(),
              "aiko.quad_warp_out: quads int32 [B, Kq, 4, 2] contiguous required");
  const int64_t Kq = quads.size(1);
  TORCH_CHECK(count.scalar_type() == at::kInt && count.dim() == 1 && count.size(0) == B && count.is_contiguous(),
              "aiko.quad_warp_out: count int32 [B] contiguous required");
  TORCH_CHECK(k >= 1 && k <= Kq, "aiko.quad_warp_out: 1 <= k <= Kq (", Kq, ") required, got ", k);
  TORCH_CHECK(margin >= 0 && margin <= 64, "aiko.quad_warp_out: margin in 0..64 (sixteenths of the side) required, "
              "got ", margin);
  TORCH_CHECK(origin == 0 || origin == 1, "aiko.quad_warp_out: origin 1 (pixel centres) or 0 (pixel edges) required, "
              "got ", origin);
  TORCH_CHECK(B * k <= 65535, "aiko.quad_warp_out: B * k = ", B * k, " slots exceed the grid limit (65535)");
  TORCH_CHECK(patches.scalar_type() == at::kByte && patches.dim() == 4 && patches.size(0) == B * k &&
                  patches.size(3) == 3 && patches.is_contiguous(),
              "aiko.quad_warp_out: patches uint8 [B*k, Ho, Wo, 3] contiguous required");
  const int64_t Ho = patches.size(1), Wo = patches.size(2);
  TORCH_CHECK(Ho >= 1 && Wo >= 4 && Wo % 4 == 0, "aiko.quad_warp_out: patch width must be a multiple of 4, got ", Wo);
  TORCH_CHECK(Ho <= 4096 && Wo <= 4096, "aiko.quad_warp_out: patch side <= 4096 required, got ", Ho, " x ", Wo);
  TORCH_CHECK(valid.scalar_type() == at::kInt && valid.dim() == 1 && valid.size(0) == B * k && valid.is_contiguous(),
              "aiko.quad_warp_out: valid int32 [B*k] contiguous required");
  TORCH_CHECK(aligned(patches, 4) && aligned(valid, 4), "aiko.quad_warp_out: patches and valid 4-byte aligned");
  // no output may overlap an input or the other output
  check_no_overlap(outs, out_names, ins, in_names, "quad_warp_out");
  check_launch(aiko_quad_warp_u8(frames.data_ptr(), quads.data_ptr<int>(), count.data_ptr<int>(), patches.data_ptr(),
                                 valid.data_ptr<int>(), (int)B, (int)H, (int)W, (int)Kq, (int)k, (int)Ho, (int)Wo,
                                 (int)margin, (int)origin, cur_stream()),
               "quad_warp_u8");
}

// out <- frames with the boxes and labels of det[b, i] (i < min(count[b], k), coordinates finite)
// drawn over them; slot b*k + i of labels / scores overrides the detector's class / score.  out may
// be frames itself (drawn in place)
void draw_detections_out(const at::Tensor& frames, const at::Tensor& det, const at::Tensor& count, int64_t k,
                         const c10::optional<at::Tensor>& labels, const c10::optional<at::Tensor>& scores,
                         const at::Tensor& names, const at::Tensor& font, const at::Tensor& palette,
                         int64_t glyph_width, int64_t thickness, int64_t text_scale, double margin, bool show_score,
                         at::Tensor& out) {
  check_cuda_all({&frames, &det, &count, &names, &font, &palette, &out},
                 {"frames", "det", "count", "names", "font", "palette", "out"});
  check_frames_u8(frames, "draw_detections_out");
  TORCH_CHECK(frames.numel() >= 3, "aiko.draw_detections_out: frames uint8 [B, H, W, 3] contiguous required");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  const int64_t max_det = check_det_count(det, count, B, "draw_detections_out");
  check_k(k, max_det, "draw_detections_out");
  const int* lp = nullptr;
  const float* sp = nullptr;
  if (labels.has_value()) {
    check_cuda(*labels, "labels");
    TORCH_CHECK(labels->scalar_type() == at::kInt && labels->dim() == 1 && labels->size(0) == B * k &&
                    labels->is_contiguous(),
                "aiko.draw_detections_out: labels int32 [B*k] required");
    lp = labels->data_ptr<int>();
  }
  if (scores.has_value()) {
    check_cuda(*scores, "scores");
    TORCH_CHECK(scores->scalar_type() == at::kFloat && scores->dim() == 1 && scores->size(0) == B * k &&
                    scores->is_contiguous(),
                "aiko.draw_detections_out: scores fp32 [B*k] required");
    sp = scores->data_ptr<float>();
  }
  TORCH_CHECK(names.scalar_type() == at::kByte && names.dim() == 2 && names.is_contiguous() && names.size(1) >= 1 &&
                  names.size(1) <= 32 && names.size(0) < (1 << 24),
              "aiko.draw_detections_out: names uint8 [C, L] contiguous with 1 <= L <= 32 required");
  TORCH_CHECK(font.scalar_type() == at::kByte && font.dim() == 2 && font.is_contiguous() && font.size(1) >= 1 &&
                  font.size(1) <= 16 && font.size(0) < (1 << 24),
              "aiko.draw_detections_out: font uint8 [G, gh] contiguous with 1 <= gh <= 16 required");
  TORCH_CHECK(glyph_width >= 1 && glyph_width <= 8, "aiko.draw_detections_out: 1 <= glyph_width <= 8 required, got ",
              glyph_width);
  TORCH_CHECK(palette.scalar_type() == at::kByte && palette.dim() == 2 && palette.size(1) == 3 &&
                  palette.is_contiguous() && palette.size(0) >= 1 && palette.size(0) < (1 << 24),
              "aiko.draw_detections_out: palette uint8 [P, 3] contiguous with P >= 1 required");
  TORCH_CHECK(thickness >= 1 && thickness <= 16, "aiko.draw_detections_out: 1 <= thickness <= 16 required, got ",
              thickness);
  TORCH_CHECK(text_scale >= 1 && text_scale <= 4, "aiko.draw_detections_out: 1 <= text_scale <= 4 required, got ",
              text_scale);
  TORCH_CHECK(margin >= 0.0 && margin <= 3.0e38, "aiko.draw_detections_out: a finite margin >= 0 required");
  TORCH_CHECK(out.scalar_type() == at::kByte && out.sizes() == frames.sizes() && out.is_contiguous(),
              "aiko.draw_detections_out: out uint8 [B, H, W, 3] contiguous, the shape of frames, required");
  check_inplace_or_disjoint(frames, out, "draw_detections_out");
  check_tile_grid(B, H, W, "draw_detections_out");
  check_launch(aiko_draw_detections(frames.data_ptr(), out.data_ptr(), det.data_ptr<float>(), count.data_ptr<int>(), lp,
                                    sp, names.data_ptr(), font.data_ptr(), palette.data_ptr(), B, H, W, max_det, k,
                                    names.size(0), names.size(1), font.size(0), font.size(1), glyph_width,
                                    palette.size(0), thickness, text_scale, (float)margin, show_score, cur_stream()),
               "draw_detections");
}

// out <- frames with the pixels inside the rects of det[b, i] (i < min(count[b], k), coordinates
// finite, class selected) replaced by the frame's mosaic (mode 0, block x block cells) or by
// fill_rgb = R | G << 8 | B << 16 (mode 1); slot b*k + i of labels overrides the detector's class,
// select[class] != 0 selects a class (no table: every class).  out may be frames itself (in place)
void redact_detections_out(const at::Tensor& frames, const at::Tensor& det, const at::Tensor& count, int64_t k,
                           const c10::optional<at::Tensor>& labels, const c10::optional<at::Tensor>& select,
                           int64_t mode, int64_t block, int64_t fill_rgb, double margin, at::Tensor& out) {
  check_cuda_all({&frames, &det, &count, &out}, {"frames", "det", "count", "out"});
  check_frames_u8(frames, "redact_detections_out");
  TORCH_CHECK(frames.numel() >= 3, "aiko.redact_detections_out: frames uint8 [B, H, W, 3] contiguous required");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  const int64_t max_det = check_det_count(det, count, B, "redact_detections_out");
  check_k(k, max_det, "redact_detections_out");
  const int* lp = nullptr;
  const void* sp = nullptr;
  int64_t C = 0;
  if (labels.has_value()) {
    check_cuda(*labels, "labels");
    TORCH_CHECK(labels->scalar_type() == at::kInt && labels->dim() == 1 && labels->size(0) == B * k &&
                    labels->is_contiguous(),
                "aiko.redact_detections_out: labels int32 [B*k] required");
    lp = labels->data_ptr<int>();
  }
  if (select.has_value()) {
    check_cuda(*select, "select");
    TORCH_CHECK(select->scalar_type() == at::kByte && select->dim() == 1 && select->size(0) >= 1 &&
                    select->size(0) < (1 << 24) && select->is_contiguous(),
                "aiko.redact_detections_out: select uint8 [C] contiguous with C >= 1 required");
    sp = select->data_ptr();
    C = select->size(0);
  }
  TORCH_CHECK(mode == 0 || mode == 1, "aiko.redact_detections_out: mode 0 (pixelate) or 1 (fill) required, got ", mode);
  TORCH_CHECK(block == 4 || block == 8 || block == 16 || block == 32,
              "aiko.redact_detections_out: block in {4, 8, 16, 32} required, got ", block);
  TORCH_CHECK(fill_rgb >= 0 && fill_rgb <= 0xffffff,
              "aiko.redact_detections_out: fill components 0..255 (packed R | G << 8 | B << 16) required, got ",
              fill_rgb);
  TORCH_CHECK(margin >= 0.0 && margin <= 3.0e38, "aiko.redact_detections_out: a finite margin >= 0 required");
  TORCH_CHECK(out.scalar_type() == at::kByte && out.sizes() == frames.sizes() && out.is_contiguous(),
              "aiko.redact_detections_out: out uint8 [B, H, W, 3] contiguous, the shape of frames, required");
  check_inplace_or_disjoint(frames, out, "redact_detections_out");
  check_tile_grid(B, H, W, "redact_detections_out");
  check_launch(aiko_redact_detections(frames.data_ptr(), out.data_ptr(), det.data_ptr<float>(), count.data_ptr<int>(),
                                      lp, sp, B, H, W, max_det, k, C, mode, block, fill_rgb, (float)margin,
                                      cur_stream()),
               "redact_detections");
}

// One tracker step (track_ops.hip; the rules are in ops/track.py): det [B, max_det, 6] / count [B] and
// the state boxes [B, T, 4] / meta [B, T, 4] / issued [B] -> the next state in boxes_out / meta_out /
// issued_out and, per ROI slot b*k + i, the track's id, its hits and the overlay's label
void track_detections_out(const at::Tensor& det, const at::Tensor& count, const at::Tensor& boxes,
                          const at::Tensor& meta, const at::Tensor& issued, int64_t k, double iou, int64_t max_age,
                          double min_score, bool class_aware, int64_t label_mod, at::Tensor& boxes_out,
                          at::Tensor& meta_out, at::Tensor& issued_out, at::Tensor& ids, at::Tensor& hits,
                          at::Tensor& labels) {
  const at::Tensor* ins[5] = {&det, &count, &boxes, &meta, &issued};
  const char* in_names[5] = {"det", "count", "boxes", "meta", "issued"};
  const at::Tensor* outs[6] = {&boxes_out, &meta_out, &issued_out, &ids, &hits, &labels};
  const char* out_names[6] = {"boxes_out", "meta_out", "issued_out", "ids", "hits", "labels"};
  check_cuda_all(ins, in_names);
  check_cuda_all(outs, out_names);
  check_same_device(ins, outs, "track_detections_out");
  TORCH_CHECK(det.scalar_type() == at::kFloat && det.dim() == 3 && det.size(2) == 6 && det.is_contiguous() &&
                  det.size(0) >= 1,
              "aiko.track_detections_out: det fp32 [B, max_det, 6] contiguous required");
  const int64_t B = det.size(0), max_det = det.size(1);
  TORCH_CHECK(count.scalar_type() == at::kInt && count.dim() == 1 && count.size(0) == B && count.is_contiguous(),
              "aiko.track_detections_out: count int32 [B] contiguous required");
  TORCH_CHECK(k >= 1 && k <= 64, "aiko.track_detections_out: 1 <= k <= 64 required, got ", k);
  TORCH_CHECK(k <= max_det, "aiko.track_detections_out: k <= max_det (", max_det, ") required, got ", k);
  TORCH_CHECK(boxes.scalar_type() == at::kFloat && boxes.dim() == 3 && boxes.size(2) == 4 && boxes.is_contiguous(),
              "aiko.track_detections_out: boxes fp32 [B, T, 4] contiguous required");
  const int64_t T = boxes.size(1);
  TORCH_CHECK(T >= 1 && T <= 64, "aiko.track_detections_out: 1 <= T <= 64 track slots required, got ", T);
  TORCH_CHECK(boxes.size(0) == B, "aiko.track_detections_out: state of ", boxes.size(0), " rows for B = ", B);
  auto is_state = [&](const at::Tensor& bx, const at::Tensor& mt, const at::Tensor& is) {
    return bx.scalar_type() == at::kFloat && bx.dim() == 3 && bx.size(0) == B && bx.size(1) == T &&
           bx.size(2) == 4 && bx.is_contiguous() && mt.scalar_type() == at::kInt && mt.dim() == 3 &&
           mt.size(0) == B && mt.size(1) == T && mt.size(2) == 4 && mt.is_contiguous() &&
           is.scalar_type() == at::kInt && is.dim() == 1 && is.size(0) == B && is.is_contiguous();
  };
  TORCH_CHECK(is_state(boxes, meta, issued), "aiko.track_detections_out: state boxes fp32 [B, T, 4], meta int32 "
              "[B, T, 4], issued int32 [B] contiguous required, B = ", B, ", T = ", T);
  TORCH_CHECK(is_state(boxes_out, meta_out, issued_out), "aiko.track_detections_out: state_out boxes fp32 [B, T, 4], "
              "meta int32 [B, T, 4], issued int32 [B] contiguous required, B = ", B, ", T = ", T);
  TORCH_CHECK(B <= 65535, "aiko.track_detections_out: B = ", B, " exceeds the grid limit (65535 rows)");
  for (const at::Tensor* t : {&ids, &hits, &labels})
    TORCH_CHECK(t->scalar_type() == at::kInt && t->dim() == 1 && t->size(0) == B * k && t->is_contiguous(),
                "aiko.track_detections_out: ids, hits and labels int32 [B*k] = [", B * k, "] contiguous required");
  TORCH_CHECK((float)iou > 0.f && (float)iou <= 1.f, "aiko.track_detections_out: 0 < iou <= 1 required, got ", iou);
  TORCH_CHECK(max_age >= 0 && max_age <= INT_MAX, "aiko.track_detections_out: max_age >= 0 required, got ", max_age);
  TORCH_CHECK(label_mod >= 1 && label_mod <= INT_MAX, "aiko.track_detections_out: label_mod >= 1 required, got ",
              label_mod);
  for (const at::Tensor* t : {&boxes, &meta, outs[0], outs[1]})
    TORCH_CHECK(aligned(*t, 16), "aiko.track_detections_out: boxes and meta 16-byte aligned");
  // no output may overlap an input or another output
  check_no_overlap(outs, out_names, ins, in_names, "track_detections_out");
  check_launch(aiko_track_detections(det.data_ptr<float>(), count.data_ptr<int>(), boxes.data_ptr<float>(),
                                     meta.data_ptr<int>(), issued.data_ptr<int>(), boxes_out.data_ptr<float>(),
                                     meta_out.data_ptr<int>(), issued_out.data_ptr<int>(), ids.data_ptr<int>(),
                                     hits.data_ptr<int>(), labels.data_ptr<int>(), (int)B, (int)max_det, (int)k, (int)T,
                                     (float)iou, (int)max_age, (float)min_score, class_aware ? 1 : 0, (int)label_mod,
                                     cur_stream()),
               "track_detections");
}

// One motion-detection step (motion_ops.hip; the rule is in ops/motion.py): frames [B, H, W, 3] and
// the state bg [B, Gh, Gw] / seen [B] -> the next state in bg_out / seen_out, the moving regions as
// detector rows in det [B, max_det, 6] / count [B], the moving cells in mask [B, Gh, Gw] and their
// number in cells [B].  Two launches on the current stream
void motion_detect_out(const at::Tensor& frames, const at::Tensor& bg, const at::Tensor& seen, int64_t cell,
                       int64_t threshold, int64_t learn_shift, bool learn_moving, int64_t warmup, int64_t min_cells,
                       at::Tensor& bg_out, at::Tensor& seen_out, at::Tensor& det, at::Tensor& count, at::Tensor& mask,
                       at::Tensor& cells) {
  const at::Tensor* ins[3] = {&frames, &bg, &seen};
  const char* in_names[3] = {"frames", "bg", "seen"};
  const at::Tensor* outs[6] = {&bg_out, &seen_out, &det, &count, &mask, &cells};
  const char* out_names[6] = {"bg_out", "seen_out", "det", "count", "mask", "cells"};
  check_cuda_all(ins, in_names);
  check_cuda_all(outs, out_names);
  check_same_device(ins, outs, "motion_detect_out");
  check_frames_u8(frames, "motion_detect_out");
  TORCH_CHECK(frames.numel() >= 3, "aiko.motion_detect_out: frames uint8 [B, H, W, 3] contiguous required");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  TORCH_CHECK(cell == 8 || cell == 16 || cell == 32, "aiko.motion_detect_out: cell in {8, 16, 32} required, got ",
              cell);
  check_tile_grid(B, H, W, "motion_detect_out");
  const int64_t Gh = (H + cell - 1) / cell, Gw = (W + cell - 1) / cell;
  TORCH_CHECK(Gh <= 255 && Gw <= 255 && Gh * Gw <= 16384, "aiko.motion_detect_out: a grid of ", Gh, " x ", Gw,
              " cells exceeds the limits (255 rows, 255 columns, 16384 cells): choose a larger cell");
  TORCH_CHECK(threshold >= 0 && threshold <= 255, "aiko.motion_detect_out: 0 <= threshold <= 255 required, got ",
              threshold);
  TORCH_CHECK(learn_shift >= 0 && learn_shift <= 8, "aiko.motion_detect_out: 0 <= learn_shift <= 8 required, got ",
              learn_shift);
  TORCH_CHECK(warmup >= 1 && warmup <= INT_MAX, "aiko.motion_detect_out: warmup >= 1 required, got ", warmup);
  TORCH_CHECK(min_cells >= 1 && min_cells <= INT_MAX, "aiko.motion_detect_out: min_cells >= 1 required, got ",
              min_cells);
  auto is_state = [&](const at::Tensor& g, const at::Tensor& s) {
    return g.scalar_type() == at::kInt && g.dim() == 3 && g.size(0) == B && g.size(1) == Gh && g.size(2) == Gw &&
           g.is_contiguous() && s.scalar_type() == at::kInt && s.dim() == 1 && s.size(0) == B && s.is_contiguous();
  };
  TORCH_CHECK(is_state(bg, seen), "aiko.motion_detect_out: state bg int32 [B, Gh, Gw], seen int32 [B] contiguous "
              "required, B = ", B, ", Gh = ", Gh, ", Gw = ", Gw);
  TORCH_CHECK(is_state(bg_out, seen_out), "aiko.motion_detect_out: state_out bg int32 [B, Gh, Gw], seen int32 [B] "
              "contiguous required, B = ", B, ", Gh = ", Gh, ", Gw = ", Gw);
  const int64_t max_det = check_det(det, B, "motion_detect_out");
  TORCH_CHECK(max_det >= 1 && max_det <= 64, "aiko.motion_detect_out: 1 <= max_det <= 64 required, got ", max_det);
  for (const at::Tensor* t : {&count, &cells})
    TORCH_CHECK(t->scalar_type() == at::kInt && t->dim() == 1 && t->size(0) == B && t->is_contiguous(),
                "aiko.motion_detect_out: count and cells int32 [B] contiguous required");
  TORCH_CHECK(mask.scalar_type() == at::kByte && mask.dim() == 3 && mask.size(0) == B && mask.size(1) == Gh &&
                  mask.size(2) == Gw && mask.is_contiguous(),
              "aiko.motion_detect_out: mask uint8 [B, Gh, Gw] = [", B, ", ", Gh, ", ", Gw, "] contiguous required");
  // no output may overlap an input or another output
  check_no_overlap(outs, out_names, ins, in_names, "motion_detect_out");
  check_launch(aiko_motion_detect(frames.data_ptr(), bg.data_ptr<int>(), seen.data_ptr<int>(), bg_out.data_ptr<int>(),
                                  seen_out.data_ptr<int>(), det.data_ptr<float>(), count.data_ptr<int>(),
                                  mask.data_ptr(), cells.data_ptr<int>(), (int)B, (int)H, (int)W, (int)cell,
                                  (int)threshold, (int)learn_shift, learn_moving ? 1 : 0, (int)warmup, (int)min_cells,
                                  (int)max_det, cur_stream()),
               "motion_detect");
}

// Square markers (marker_ops.hip; the rule is in ops/marker.py): frames [B, H, W, 3] -> the markers as
// detector rows in det [B, max_det, 6] / count [B], their quads in corners [B, max_det, 4, 2], their ids in
// ids [B, max_det], the candidates' number in cands [B] and the on cells in mask [B, Gh, Gw]; work int32
// [>= B (H ceil(W / 32) + ceil(H / 16) ceil(W / 16))] is the workspace.  modules = 7 (original) or 6
// (payload16).  passes: 7, or the bits of the passes to launch alone (measurements).  Three launches on
// the current stream
void marker_detect_out(const at::Tensor& frames, int64_t modules, int64_t cell, int64_t contrast, int64_t min_side,
                       int64_t max_cand, int64_t passes, at::Tensor& det, at::Tensor& count, at::Tensor& corners,
                       at::Tensor& ids, at::Tensor& cands, at::Tensor& mask, at::Tensor& work) {
  const at::Tensor* outs[7] = {&det, &count, &corners, &ids, &cands, &mask, &work};
  const char* out_names[7] = {"det", "count", "corners", "ids", "cands", "mask", "work"};
  check_cuda(frames, "frames");
  for (int o = 0; o < 7; ++o) {
    check_cuda(*outs[o], out_names[o]);
    check_same_device({&frames}, {outs[o]}, "marker_detect_out");
  }
  check_frames_u8(frames, "marker_detect_out");
  TORCH_CHECK(frames.numel() >= 3, "aiko.marker_detect_out: frames uint8 [B, H, W, 3] contiguous required");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  TORCH_CHECK(modules == 6 || modules == 7, "aiko.marker_detect_out: modules 7 (original) or 6 (payload16) required, "
              "got ", modules);
  TORCH_CHECK(cell == 4 || cell == 8 || cell == 16, "aiko.marker_detect_out: cell in {4, 8, 16} required, got ", cell);
  TORCH_CHECK(B <= 65535 && H <= 4096 && W <= 4096, "aiko.marker_detect_out: B = ", B, ", H = ", H, ", W = ", W,
              " exceed the frame limits (65535 frames, 4096 pixels a side)");
  const int64_t Gh = (H + cell - 1) / cell, Gw = (W + cell - 1) / cell;
  TORCH_CHECK((Gh + 2) * (Gw + 2) <= 36864, "aiko.marker_detect_out: a grid of ", Gh, " x ", Gw,
              " cells exceeds the limit ((Gh + 2) (Gw + 2) <= 36864): choose a larger cell");
  TORCH_CHECK(contrast >= 1 && contrast <= 255, "aiko.marker_detect_out: 1 <= contrast <= 255 required, got ",
              contrast);
  TORCH_CHECK(min_side >= 1 && min_side <= 4096, "aiko.marker_detect_out: 1 <= min_side <= 4096 required, got ",
              min_side);
  TORCH_CHECK(max_cand >= 1 && max_cand <= 64, "aiko.marker_detect_out: 1 <= max_cand <= 64 required, got ",
              max_cand);
  TORCH_CHECK(passes >= 1 && passes <= 7, "aiko.marker_detect_out: passes in 1..7 required, got ", passes);
  const int64_t max_det = check_det(det, B, "marker_detect_out");
  TORCH_CHECK(max_det >= 1 && max_det <= 64, "aiko.marker_detect_out: 1 <= max_det <= 64 required, got ", max_det);
  for (const at::Tensor* t : {&count, &cands})
    TORCH_CHECK(t->scalar_type() == at::kInt && t->dim() == 1 && t->size(0) == B && t->is_contiguous(),
                "aiko.marker_detect_out: count and cands int32 [B] contiguous required");
  TORCH_CHECK(corners.scalar_type() == at::kInt && corners.dim() == 4 && corners.size(0) == B &&
                  corners.size(1) == max_det && corners.size(2) == 4 && corners.size(3) == 2 && corners.is_contiguous(),
              "aiko.marker_detect_out: corners int32 [B, max_det, 4, 2] = [", B, ", ", max_det,
              ", 4, 2] contiguous required");
  TORCH_CHECK(ids.scalar_type() == at::kInt && ids.dim() == 2 && ids.size(0) == B && ids.size(1) == max_det &&
                  ids.is_contiguous(),
              "aiko.marker_detect_out: ids int32 [B, max_det] = [", B, ", ", max_det, "] contiguous required");
  TORCH_CHECK(mask.scalar_type() == at::kByte && mask.dim() == 3 && mask.size(0) == B && mask.size(1) == Gh &&
                  mask.size(2) == Gw && mask.is_contiguous(),
              "aiko.marker_detect_out: mask uint8 [B, Gh, Gw] = [", B, ", ", Gh, ", ", Gw, "] contiguous required");
  const int64_t need = B * (H * ((W + 31) / 32) + ((H + 15) / 16) * ((W + 15) / 16));
  TORCH_CHECK(work.scalar_type() == at::kInt && work.dim() == 1 && work.size(0) >= need && work.is_contiguous(),
              "aiko.marker_detect_out: work int32 [>= ", need, "] contiguous required");
  // no output may overlap the frames or another output
  check_no_overlap(outs, out_names, {&frames}, {"frames"}, "marker_detect_out");
  check_launch(aiko_marker_detect(frames.data_ptr(), det.data_ptr<float>(), count.data_ptr<int>(),
                                  corners.data_ptr<int>(), ids.data_ptr<int>(), cands.data_ptr<int>(), mask.data_ptr(),
                                  work.data_ptr(), (int)B, (int)H, (int)W, (int)modules, (int)cell, (int)contrast,
                                  (int)min_side, (int)max_cand, (int)max_det, (int)passes, cur_stream()),
               "marker_detect");
}

// The camera wall (wall_ops.hip; the rule is in ops/wall.py): frames [B, H, W, 3] and, optionally,
// score int32 [B] -> wall [P, rows tile_h + (rows + 1) gap, cols tile_w + (cols + 1) gap, 3] and the
// camera of every tile in source [P, rows cols].  order 0 index, 1 score.  Colours are packed
// R | G << 8 | B << 16.  passes: 3, or the bits of the launches to run alone (measurements: 1 the
// selection, 2 the composition from the source the caller filled).  Two launches on the current stream
void frame_wall_out(const at::Tensor& frames, const c10::optional<at::Tensor>& score, int64_t rows, int64_t cols,
                    int64_t tile_h, int64_t tile_w, int64_t gap, int64_t order, int64_t min_score, int64_t ring,
                    int64_t label_scale, int64_t label_base, int64_t background, int64_t alert, int64_t label_fg,
                    int64_t label_bg, int64_t passes, at::Tensor& wall, at::Tensor& source) {
  check_cuda_all({&frames, &wall, &source}, {"frames", "wall", "source"});
  check_same_device({&frames}, {&wall, &source}, "frame_wall_out");
  check_frames_u8(frames, "frame_wall_out");
  TORCH_CHECK(frames.numel() >= 3, "aiko.frame_wall_out: frames uint8 [B, H, W, 3] contiguous required");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  TORCH_CHECK(B <= INT_MAX && H * W <= (1 << 23), "aiko.frame_wall_out: H * W = ", H * W,
              " exceeds 2^23 pixels per frame (the 32-bit sums of the area average)");
  TORCH_CHECK(rows >= 1 && cols >= 1 && rows * cols <= 1024, "aiko.frame_wall_out: rows, cols >= 1 and rows * cols "
              "<= 1024 tiles per page required, got ", rows, " x ", cols);
  TORCH_CHECK(tile_h >= 1 && tile_h <= H && tile_w >= 1 && tile_w <= W, "aiko.frame_wall_out: a tile of 1..", H,
              " x 1..", W, " required (the wall never enlarges), got ", tile_h, " x ", tile_w);
  TORCH_CHECK(gap >= 0 && gap <= 64, "aiko.frame_wall_out: 0 <= gap <= 64 required, got ", gap);
  TORCH_CHECK(order == 0 || order == 1, "aiko.frame_wall_out: order 0 (index) or 1 (score) required, got ", order);
  TORCH_CHECK(min_score >= INT_MIN && min_score <= INT_MAX, "aiko.frame_wall_out: min_score must fit int32");
  TORCH_CHECK(ring >= 0 && 2 * ring <= std::min(tile_h, tile_w), "aiko.frame_wall_out: 0 <= 2 ring <= min(tile) "
              "required, got ring ", ring);
  TORCH_CHECK(label_scale >= 0 && label_scale <= 4, "aiko.frame_wall_out: 0 <= label_scale <= 4 required, got ",
              label_scale);
  TORCH_CHECK(label_base >= 0 && label_base + B <= INT_MAX, "aiko.frame_wall_out: label_base >= 0 with label_base + "
              "B <= 2^31 - 1 required, got ", label_base);
  for (int64_t c : {background, alert, label_fg, label_bg})
    TORCH_CHECK(c >= 0 && c <= 0xffffff, "aiko.frame_wall_out: colour components 0..255 (packed R | G << 8 | B << "
                "16) required, got ", c);
  TORCH_CHECK(passes >= 1 && passes <= 3, "aiko.frame_wall_out: passes in 1..3 required, got ", passes);
  const int* score_p = nullptr;
  if (defined(score)) {
    check_cuda(*score, "score");
    check_same_device({&frames}, {&*score}, "frame_wall_out");
    TORCH_CHECK(score->scalar_type() == at::kInt && score->dim() == 1 && score->size(0) == B && score->is_contiguous(),
                "aiko.frame_wall_out: score int32 [B] = [", B, "] contiguous required");
    score_p = score->data_ptr<int>();
  }
  TORCH_CHECK(order == 0 || score_p, "aiko.frame_wall_out: score order requires a score");
  TORCH_CHECK(order == 0 || B <= 4096, "aiko.frame_wall_out: score order ranks at most 4096 cameras, got ", B);
  const int64_t N = rows * cols;
  const int64_t Hw = rows * tile_h + (rows + 1) * gap, Ww = cols * tile_w + (cols + 1) * gap;
  TORCH_CHECK(wall.scalar_type() == at::kByte && wall.dim() == 4 && wall.size(0) >= 1 && wall.size(1) == Hw &&
                  wall.size(2) == Ww && wall.size(3) == 3 && wall.is_contiguous(),
              "aiko.frame_wall_out: wall uint8 [P >= 1, ", Hw, ", ", Ww, ", 3] contiguous required");
  const int64_t P = wall.size(0);
  TORCH_CHECK(Hw <= (1 << 24) && Ww <= (1 << 24) && P * N < (1 << 24), "aiko.frame_wall_out: a wall of ", P, " x ", Hw,
              " x ", Ww, " exceeds the limits (side <= 2^24, pages * tiles < 2^24)");
  TORCH_CHECK(source.scalar_type() == at::kInt && source.dim() == 2 && source.size(0) == P && source.size(1) == N &&
                  source.is_contiguous(),
              "aiko.frame_wall_out: source int32 [P, rows * cols] = [", P, ", ", N, "] contiguous required");
  // no output may overlap an input or the other output
  if (score_p)
    check_no_overlap({&wall, &source}, {"wall", "source"}, {&frames, &*score}, {"frames", "score"}, "frame_wall_out");
  else
    check_no_overlap({&wall, &source}, {"wall", "source"}, {&frames}, {"frames"}, "frame_wall_out");
  check_launch(aiko_frame_wall(frames.data_ptr(), score_p, source.data_ptr<int>(), wall.data_ptr(), (int)B, (int)H,
                               (int)W, (int)rows, (int)cols, (int)tile_h, (int)tile_w, (int)gap, (int)P, (int)order,
                               (int)min_score, (int)ring, (int)label_scale, (int)label_base, (int)background,
                               (int)alert, (int)label_fg, (int)label_bg, (int)passes, cur_stream()),
               "frame_wall");
}

}  // namespace

TORCH_LIBRARY_IMPL(aiko, CUDA, m) {
  m.impl("yolo_decode_out", &yolo_decode_out);
  m.impl("topk_nms_out", &topk_nms_out);
  m.impl("roi_crop_out", &roi_crop_out);
  m.impl("quad_warp_out", &quad_warp_out);
  m.impl("draw_detections_out", &draw_detections_out);
  m.impl("redact_detections_out", &redact_detections_out);
  m.impl("track_detections_out", &track_detections_out);
  m.impl("motion_detect_out", &motion_detect_out);
  m.impl("marker_detect_out", &marker_detect_out);
  m.impl("frame_wall_out", &frame_wall_out);
}
