// The operator schemas of torch.ops.aiko.*: the one TORCH_LIBRARY block.  The implementations and
// their TORCH_LIBRARY_IMPL blocks are in this directory's other files, one per domain.
#include <torch/library.h>

TORCH_LIBRARY(aiko, m) {
  m.def("conv_igemm_out(Tensor x, Tensor? x2, Tensor w, Tensor? bias, Tensor? res, Tensor(a!) y, int[] geom, Tensor? zero=None) -> ()");
  m.def("preprocess_out(Tensor frames, Tensor(a!) out, int Ho, int Wo, int pad_t, int pad_l, float[] mean, float[] std, bool bgr, float[] canvas=[]) -> ()");
  m.def("upsample2x_out(Tensor x, Tensor(a!) y) -> ()");
  m.def("resize_u8_out(Tensor x, Tensor(a!) y) -> ()");
  m.def("scale_frames_out(Tensor frames, Tensor? hb, Tensor? hk, Tensor? vb, Tensor? vk, int tile_rows, int tile_cols, int win_rows, Tensor(a!) out) -> ()");
  m.def("roi_crop_out(Tensor frames, Tensor det, Tensor count, int k, float margin, Tensor(a!) crops, Tensor(b!) rois) -> ()");
  m.def("quad_warp_out(Tensor frames, Tensor quads, Tensor count, int k, int margin, int origin, Tensor(a!) patches, Tensor(b!) valid) -> ()");
  m.def("draw_detections_out(Tensor frames, Tensor det, Tensor count, int k, Tensor? labels, Tensor? scores, Tensor names, Tensor font, Tensor palette, int glyph_width, int thickness, int text_scale, float margin, bool show_score, Tensor(a!) out) -> ()");
  m.def("redact_detections_out(Tensor frames, Tensor det, Tensor count, int k, Tensor? labels, Tensor? select, int mode, int block, int fill_rgb, float margin, Tensor(a!) out) -> ()");
  m.def("yuv_to_rgb_out(Tensor raw, int height, int width, int format, float[] coeffs, int round_mode, Tensor(a!) out) -> ()");
  m.def("rgb_to_yuv_out(Tensor rgb, int fmt, float[] coeffs, int round, Tensor(a!) out) -> ()");
  m.def("batchnorm_out(Tensor x, Tensor scale, Tensor shift, Tensor(a!) y, int act) -> ()");
  m.def("yolo_decode_out(Tensor[] feats, int[] strides, int nc, int reg_max, Tensor(a!) boxes, Tensor(b!) scores, Tensor(c!) cls) -> ()");
  m.def("topk_nms_out(Tensor boxes, Tensor scores, Tensor cls, int max_cand, float[] params, Tensor(a!) det, Tensor(b!) count) -> ()");
  m.def("stem_direct_out(Tensor frames, Tensor w, Tensor? bias, Tensor(a!) out, int[] geom, float fill, float[] mean, float[] std, bool bgr) -> ()");
  m.def("conv3x3_patch_out(Tensor x, Tensor wimg, Tensor? bias, Tensor(a!) y, int act, int grid=0) -> ()");
  m.def("conv3x3_patchw_out(Tensor x, Tensor wimg, Tensor? bias, Tensor(a!) y, int act, int grid=0) -> ()");
  m.def("conv3x3_rows_out(Tensor x, Tensor wimg, Tensor? bias, Tensor? res, Tensor(a!) y, int act, int grid=0) -> ()");
  m.def("conv_chain_out(Tensor A, Tensor W1, Tensor b1, Tensor? R, Tensor(a!) Y, Tensor W2, Tensor b2, Tensor(b!) Z, int grid=0, Tensor? A2=None) -> ()");
  m.def("bneck_fused_out(Tensor x, Tensor w1, Tensor b1, Tensor w2, Tensor b2, Tensor w3, Tensor b3, Tensor(a!) y, int grid=0, Tensor? dbg=None) -> ()");
  m.def("conv3x3_exp_out(Tensor t1, Tensor w2, Tensor b2, Tensor w3, Tensor b3, Tensor res, Tensor(a!) y, int grid=0) -> ()");
  m.def("maxpool_out(Tensor x, Tensor(a!) y, int k, int s, int p) -> ()");
  m.def("avgpool_out(Tensor x, Tensor(a!) y) -> ()");
  m.def("mean_rows_out(Tensor x, Tensor(a!) y) -> ()");
  m.def("window_shift_out(Tensor src, Tensor chunk, Tensor(a!) dst) -> ()");
  m.def("track_detections_out(Tensor det, Tensor count, Tensor boxes, Tensor meta, Tensor issued, int k, float iou, int max_age, float min_score, bool class_aware, int label_mod, Tensor(a!) boxes_out, Tensor(b!) meta_out, Tensor(c!) issued_out, Tensor(d!) ids, Tensor(e!) hits, Tensor(f!) labels) -> ()");
  m.def("marker_detect_out(Tensor frames, int modules, int cell, int contrast, int min_side, int max_cand, int passes, Tensor(a!) det, Tensor(b!) count, Tensor(c!) corners, Tensor(d!) ids, Tensor(e!) cands, Tensor(f!) mask, Tensor(g!) work) -> ()");
  m.def("motion_detect_out(Tensor frames, Tensor bg, Tensor seen, int cell, int threshold, int learn_shift, bool learn_moving, int warmup, int min_cells, Tensor(a!) bg_out, Tensor(b!) seen_out, Tensor(c!) det, Tensor(d!) count, Tensor(e!) mask, Tensor(f!) cells) -> ()");
  m.def("frame_wall_out(Tensor frames, Tensor? score, int rows, int cols, int tile_h, int tile_w, int gap, int order, int min_score, int ring, int label_scale, int label_base, int background, int alert, int label_fg, int label_bg, int passes, Tensor(a!) wall, Tensor(b!) source) -> ()");
  m.def("voice_activity_out(Tensor audio, Tensor state, int frame, int threshold, int min_level, int up_shift, int speech_shift, int down_shift, int warmup, int attack, int hang, int max_zc, int window, Tensor(a!) state_out, Tensor(b!) level, Tensor(c!) zc, Tensor(d!) mask, Tensor(e!) seg, Tensor(f!) count, Tensor(g!) speech, Tensor(h!) silent) -> ()");
  m.def("spectrum_out(Tensor audio, Tensor window, Tensor twiddle, Tensor band_start, int n_fft, int hop, float inv_F, float lo, float hi, int k_lo, int k_hi, bool local, Tensor(a!) power, Tensor(b!) amplitudes, Tensor(c!) band_amplitudes, Tensor(d!) peak_bins, Tensor(e!) peak_amplitudes, Tensor(f!) peak_counts) -> ()");
  m.def("spectrum_graph_out(Tensor peak_bins, Tensor peak_amplitudes, Tensor peak_counts, Tensor bin_px, float y_max, int[] color, Tensor(a!) image) -> ()");
  m.def("jpeg_encode_out(Tensor raw, int height, int width, int fmt, Tensor tables, int header_len, int seg_cap, Tensor(a!) stream, Tensor(b!) nbytes, Tensor(c!) workspace) -> ()");
  m.def("jpeg_decode_out(Tensor data, Tensor nbytes, Tensor desc, int height, int width, int fmt, int max_intervals, Tensor(a!) raw, Tensor(b!) status, Tensor(c!) workspace) -> ()");
  m.def("resample_out(Tensor pcm, Tensor hist, Tensor filt, int L, int M, Tensor(a!) out, Tensor(b!) hist_out) -> ()");
  m.def("zero_border_rows_(Tensor(a!) x, int rows) -> ()");
  m.def("sppf_pool_(Tensor(a!) cat, int c, int k) -> ()");
  m.def("stem_pool_out(Tensor x, Tensor w, Tensor bias, Tensor(a!) y, int Ho, int Wo, int variant=0) -> ()");
  m.def("stem_pool_u8_out(Tensor frames, Tensor w, Tensor bias, Tensor(a!) y, float[] mean255, int variant=0) -> ()");
  m.def("gemm_fp8_out(Tensor a, Tensor? sa, Tensor b, Tensor sb, Tensor? bias, Tensor? res, Tensor(a!)? y, int act, int bm, int bn, int variant=0, Tensor? zero=None, Tensor? amx=None, Tensor(b!)? yq=None, Tensor(c!)? ysc=None) -> ()");
  m.def("rownorm_quant_out(Tensor x, Tensor? gamma, Tensor? beta, float eps, Tensor(a!)? yb, Tensor(b!)? q, Tensor(c!)? qs) -> ()");
  m.def("c2f_fused_out(Tensor x, Tensor w1, Tensor b1, Tensor wa, Tensor ba, Tensor wb, Tensor bb, Tensor w2, Tensor b2, Tensor(a!) y, int ci, bool shortcut, int rb, Tensor? xu=None) -> ()");
  m.def("c2f_bneck_out(Tensor x, Tensor wa, Tensor ba, Tensor wb, Tensor bb, Tensor(a!) y, bool shortcut, int rb) -> ()");
  m.def("conv_glds_tail_decode_out(Tensor x, Tensor w, Tensor bias, Tensor w2, Tensor b2, Tensor(a!) boxes, Tensor(b!) scores, Tensor(c!) cls, int R, int pad, int act, int mode, int nc, int level_stride, int astart, Tensor zero) -> ()");
  m.def("conv_glds_tail_out(Tensor x, Tensor w, Tensor bias, Tensor w2, Tensor b2, Tensor(a!) y2, int R, int stride, int pad, int act, int act2, Tensor zero) -> ()");
  m.def("linear_splitk_out(Tensor x, Tensor w, Tensor? bias, Tensor(a!) part, Tensor(b!) y, int K, int S) -> ()");
  m.def("attn_fwd_out(Tensor q, Tensor k, Tensor v, Tensor(a!) o, int B, int H, int T, int Tpad, float scale, Tensor(b!)? work=None, Tensor(c!)? oq=None, Tensor(d!)? osc=None) -> ()");
  m.def("logmel_out(Tensor audio, Tensor mel, Tensor mel_range, int n_fft, int hop, int F, Tensor(a!) work, Tensor(b!) gmax, Tensor(c!) dst, int rows, int pad) -> ()");
  m.def("softmax_topk_out(Tensor logits, Tensor(a!) prob, Tensor(b!) index, int k) -> ()");
  m.def("embed_tokens_out(Tensor ids, Tensor pos, Tensor tok, Tensor pemb, Tensor(a!) x) -> ()");
  m.def("attn_decode_out(Tensor q, Tensor(a!) k, Tensor(b!) v, Tensor(c!) o, int B, int H, int S, int T, Tensor? pos, Tensor? knew, Tensor? vnew, float scale, Tensor(d!) work) -> ()");
  m.def("dec_linear_out(Tensor x, Tensor? gamma, Tensor? beta, float eps, Tensor w, Tensor sw, Tensor? bias, Tensor? res, Tensor(a!) y, int act) -> ()");
  m.def("argmax_step_out(Tensor logits, int V, Tensor(a!) ids, Tensor(b!) pos, Tensor(c!) out_tokens, Tensor forced, int eot, Tensor(d!) done, Tensor(e!) counter) -> ()");
}
