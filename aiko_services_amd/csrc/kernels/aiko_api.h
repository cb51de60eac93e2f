// The host entry points of the kernel files: the one declaration of every extern "C" aiko_*
// launcher.  Every .hip file that defines or calls one includes this header, and so do the torch
// bindings (csrc/bindings/), so a prototype that disagrees with its definition is a compile error
// in the kernel file instead of shifted arguments at run time.  The launchers return 0, a
// hipError_t (> 0) or -1 for a configuration they do not cover; none allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>

#include "conv_launch.h"

extern "C" {

// ---- conv_igemm.hip / conv_glds.hip / conv_buf.hip / conv_persist.hip / conv_wide.hip:
//      the variants of the implicit-GEMM conv (ConvLaunch: conv_launch.h)
int aiko_conv_igemm(const ConvLaunch* l);
int aiko_conv_glds(const ConvLaunch* l, const void* zero);
int aiko_conv_glds_tail(const void* x, const void* w, const float* bias, int H, int W, int C, int Cc, int R, int S,
                        int stride, int pad, int Ho, int Wo, int M, int K, int N, int act, const void* w2, const float* b2,
                        void* y2, int ldy2, int ldw2, int act2, const void* zero, const int* dec, void* boxes,
                        float* scores, int* cls, hipStream_t stream);
int aiko_conv_buf(const ConvLaunch* l, int occ, int mf32);
int aiko_conv_persist(const ConvLaunch* l);
int aiko_conv_wide(const ConvLaunch* l, int occ);

// ---- conv_pw.hip: 1x1 convs with streamed or resident weights
int aiko_conv_pw(const void* x, const void* w, const float* bias, const void* res, void* y, int M, int N,
                 int K, int ldx, int ldy, int ldr, int act, int cus, int mode, hipStream_t stream);
int aiko_conv_pw_dual(const void* x, const void* x2, const void* w, const float* bias, void* y, int M, int N,
                      int ldx, int ldx2, int ldy, int act, int Ho, int Wo, int H2, int W2, int s2, int cus,
                      hipStream_t stream);

// ---- conv_narrow.hip: 16 / 32-channel convs
int aiko_conv_narrow(const void* x, const void* w, const float* bias, const void* res, void* y, int H, int W, int C,
                     int Cc, int R, int S, int stride, int pad, int Ho, int Wo, int M, int Cout, int K, int act,
                     int ldy, int ldr, int th, int wreg, hipStream_t stream);

// ---- conv_patch.hip / conv_patchw.hip / conv_rows.hip: 3x3 convs with an LDS-resident input
int aiko_conv3x3_patch(const void* x, const void* wimg, const float* bias, void* y, int B, int H, int W, int ldy,
                       int act, int grid, hipStream_t stream);
int aiko_conv3x3_patchw(const void* x, const void* wimg, const float* bias, void* y, int B, int H, int W, int ldx,
                        int ldy, int act, int grid, hipStream_t stream);
int aiko_conv3x3_rows(const void* x, const void* wimg, const float* bias, const void* res, void* y, int B, int H,
                      int W, int ldx, int ldy, int ldr, int act, int grid, hipStream_t stream);

// ---- conv_chain.hip / conv_chain2.hip: chained 1x1 convs (aiko_conv_chain calls aiko_conv_chain2)
int aiko_conv_chain(const void* A, const void* W1, const float* b1, const void* R, void* Y, const void* W2,
                    const float* b2, void* Z, const void* A2, int M, int K1, int N1, int N2, int grid,
                    hipStream_t stream);
int aiko_conv_chain2(const void* A, const void* W1, const float* b1, const void* R, void* Y, const void* W2,
                     const float* b2, void* Z, int M, int K1, int N1, int N2, int grid, hipStream_t stream);

// ---- bneck_fused.hip / conv_exp.hip / c2f_fused.hip: whole blocks in one launch
int aiko_bneck_fused(const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                     const void* w3, const float* b3, void* y, int B, int H, int W, int cin, int grid,
                     unsigned* dbg, hipStream_t stream);
int aiko_conv3x3_exp(const void* t1, const void* w2, const float* b2, const void* w3img, const float* b3,
                     const void* res, void* y, int B, int H, int W, int N, int grid, hipStream_t stream);
int aiko_c2f_fused(const void* x, int ldx, const void* w1, const float* b1, int k1, const void* wa, const float* ba,
                   int ka, const void* wb, const float* bb, int kb, const void* w2, const float* b2, int k2, void* y, int ldy,
                   int B, int H, int W, int CI, int C, int CO, int shortcut, int rb, const void* xu, int ldxu, int cu, hipStream_t stream);
int aiko_c2f_bneck(const void* x, int ldx, const void* wa, const float* ba, int ka, const void* wb, const float* bb,
                   int kb, void* y, int ldy, int B, int H, int W, int C, int shortcut, int rb, hipStream_t stream);

// ---- stem_pool.hip: 7x7 stem conv + max-pool from the bf16 stem buffer or from uint8 frames
int aiko_stem_pool(const void* x, const void* w, const float* bias, void* y, int B, int Hp, int Wp,
                   int Ho, int Wo, int Hm, int Wm, int ldy, int variant, hipStream_t stream);
int aiko_stem_pool_u8(const void* frames, const void* w, const float* bias, void* y, int B, int Hi, int Wi,
                      int Ho, int Wo, int Hm, int Wm, int ldy, const float* mean255, int variant, hipStream_t stream);

// ---- vision_ops.hip: pre-processing, pools and the classifier's tail
int aiko_resize_u8(const void* in, void* out, int B, int Hin, int Win, int Ho, int Wo, hipStream_t stream);
int aiko_batchnorm(const void* x, void* y, const float* scale, const float* shift, long P, int C, int ldx,
                   int ldy, int act, hipStream_t stream);
int aiko_preprocess(const void* in, void* out, int B, int Hin, int Win, int Ho, int Wo, int Hp,
                    int Wp, int pad_t, int pad_l, int Hc, int Wc, int off_t, int off_l, float fill,
                    const float* mean, const float* std, int bgr, hipStream_t stream);
int aiko_stem_direct(const void* in, void* out, const void* w, const float* bias, int B, int Hin, int Win,
                     int Ho, int Wo, int Hc, int Wc, int off_t, int off_l, float fill, const float* mean,
                     const float* std, int bgr, int H1, int W1, int Cout, int ldo, int k, int stride, int pad,
                     int act, hipStream_t stream);
int aiko_maxpool(const void* x, void* y, int B, int H, int W, int C, int Ho, int Wo, int k,
                 int s, int p, int ldx, int ldy, hipStream_t stream);
int aiko_mean_rows_f32(const void* x, float* y, int B, int T, int C, long ldb, hipStream_t stream);
int aiko_avgpool(const void* x, void* y, int B, int HW, int C, hipStream_t stream);
int aiko_softmax_topk(const void* logits, float* prob, int* index, int B, int N, int k,
                      hipStream_t stream);
int aiko_sppf_pool(void* x, int B, int H, int W, int ld, int c, int k, hipStream_t stream);
int aiko_zero_border_rows(void* x, int B, int rows, int C, hipStream_t stream);

// ---- detect_ops.hip: the detect head's tail (aiko_topk_nms_groups: workgroups per image)
int aiko_upsample2x(const void* x, void* y, int B, int H, int W, int C, int ldx, int ldy,
                    hipStream_t stream);
int aiko_yolo_decode(const void* const* feats, const int* H, const int* W, const int* strides,
                     const int* ld, int nlev, int B, int nc, int reg_max, void* boxes,
                     float* scores, int* cls, hipStream_t stream);
int aiko_topk_nms_groups(int B);
size_t aiko_topk_nms_workspace(int B);
int aiko_topk_nms(const void* boxes, const float* scores, const int* cls, int B, int A,
                  int max_cand, int max_det, float conf, float iou, float max_wh, float gain,
                  float pad_l, float pad_t, float img_w, float img_h, float* det, int* count,
                  void* workspace, hipStream_t stream);

// ---- roi_ops.hip / overlay_ops.hip / redact_ops.hip: crop, draw and redact detections
int aiko_roi_crop_u8(const void* frames, const float* det, const int* count, void* crops, int* rois, int B, int H,
                     int W, int max_det, int K, int Ho, int Wo, float margin, hipStream_t stream);
int aiko_draw_detections(const void* frames, void* out, const float* det, const int* count, const int* labels,
                         const float* scores, const void* names, const void* font, const void* palette, int B, int H,
                         int W, int max_det, int K, int C, int L, int G, int gh, int gw, int P, int t, int s,
                         float margin, int show_score, hipStream_t stream);
int aiko_redact_detections(const void* frames, void* out, const float* det, const int* count, const int* labels,
                           const void* select, int B, int H, int W, int max_det, int K, int C, int mode, int block,
                           int fill_rgb, float margin, hipStream_t stream);

// ---- track_ops.hip: one tracker step
int aiko_track_detections(const float* det, const int* count, const float* boxes, const int* meta, const int* issued,
                          float* boxes_out, int* meta_out, int* issued_out, int* ids, int* hits, int* labels, int B,
                          int max_det, int K, int T, float thr, int max_age, float min_score, int class_aware,
                          int label_mod, hipStream_t stream);

// ---- motion_ops.hip: one motion-detection step (aiko_motion_detect = the cell pass + the region pass)
int aiko_motion_cells(const void* frames, const int* bg, const int* seen, int* bg_out, int* seen_out, void* mask,
                      int B, int H, int W, int cell, int threshold, int learn_shift, int learn_moving, int warmup,
                      hipStream_t stream);
int aiko_motion_regions(const void* mask, float* det, int* count, int* cells, int B, int H, int W, int cell,
                        int min_cells, int max_det, hipStream_t stream);
int aiko_motion_detect(const void* frames, const int* bg, const int* seen, int* bg_out, int* seen_out, float* det,
                       int* count, void* mask, int* cells, int B, int H, int W, int cell, int threshold,
                       int learn_shift, int learn_moving, int warmup, int min_cells, int max_det, hipStream_t stream);

// ---- wall_ops.hip: the camera wall (aiko_frame_wall = the selection + the composition)
int aiko_wall_select(const int* score, int* source, int B, long slots, int order, int min_score, hipStream_t stream);
int aiko_wall_compose(const void* frames, const int* score, const int* source, void* wall, int B, int H, int W, int R,
                      int C, int th, int tw, int g, int P, int min_score, int ring, int label_scale, int label_base,
                      int background, int alert, int label_fg, int label_bg, hipStream_t stream);
int aiko_frame_wall(const void* frames, const int* score, int* source, void* wall, int B, int H, int W, int R, int C,
                    int th, int tw, int g, int P, int order, int min_score, int ring, int label_scale, int label_base,
                    int background, int alert, int label_fg, int label_bg, int passes, hipStream_t stream);

// ---- scale_ops.hip: the antialiased fixed-point resize (null bounds = that pass is left out)
int aiko_scale_frames(const void* frames, const int* hb, const int* hk, const int* vb, const int* vk, void* out, int B,
                      int H, int W, int Ho, int Wo, int ksh, int ksv, int tile_rows, int tile_cols, int win_rows,
                      hipStream_t stream);

// ---- marker_ops.hip: square markers
int aiko_marker_detect(const void* frames, float* det, int* count, int* corners, int* ids, int* cands, void* mask,
                       void* work, int B, int H, int W, int N, int cell, int contrast, int min_side, int max_cand,
                       int max_det, int passes, hipStream_t stream);

// ---- warp_ops.hip: projective warp selected by quads
int aiko_quad_warp_u8(const void* frames, const int* quads, const int* count, void* patches, int* valid, int B, int H,
                      int W, int Kq, int K, int Ho, int Wo, int margin, int origin, hipStream_t stream);

// ---- yuv_ops.hip / yuv_out_ops.hip: raw YUV frames in and out
int aiko_yuv_to_rgb_u8(const void* raw, void* out, int B, int H, int W, int fmt, const float* coef, int half,
                       hipStream_t stream);
int aiko_rgb_to_yuv_u8(const void* rgb, void* out, int B, int H, int W, int fmt, const float* coef, int half,
                       hipStream_t stream);

// ---- jpeg_ops.hip: baseline JPEG encoding (aiko_jpeg_encode = the row pass + the assembly)
int aiko_jpeg_rows(const void* raw, const void* tables, void* workspace, int B, int H, int W, int fmt, int seg_cap,
                   hipStream_t strm);
int aiko_jpeg_assemble(const void* tables, int header_len, const void* workspace, void* stream, int* nbytes, int B,
                       int H, int W, int fmt, long cap, int seg_cap, hipStream_t strm);
int aiko_jpeg_encode(const void* raw, const void* tables, int header_len, void* workspace, void* stream, int* nbytes,
                     int B, int H, int W, int fmt, long cap, int seg_cap, hipStream_t strm);

// ---- jpeg_decode_ops.hip: baseline JPEG decoding (pass 0 the marker scan, 1 the entropy decode, 2 the IDCT)
int aiko_jpeg_decode_pass(int pass, const void* data, const int* nbytes, const void* desc, int desc_rows,
                          void* workspace, void* raw, int* status, int B, int H, int W, int fmt, long cap, int max_int,
                          hipStream_t strm);
int aiko_jpeg_decode(const void* data, const int* nbytes, const void* desc, int desc_rows, void* workspace, void* raw,
                     int* status, int B, int H, int W, int fmt, long cap, int max_int, hipStream_t strm);

// ---- resample_ops.hip / vad_ops.hip / spectrum_ops.hip / audio_ops.hip: audio
int aiko_resample(const void* pcm, int is_f32, const float* hist, const float* filt, float* out, float* hist_out,
                  int B, long n_in, int C, int L, int M, int T, hipStream_t stream);
int aiko_vad_frames(const float* audio, int* level, int* zc, int B, int F, int frame, hipStream_t stream);
int aiko_vad_stream(const int* level, const int* zc, const int* state, int* state_out, void* mask, int* seg,
                    int* count, int* speech, int* silent, int B, int F, int frame, int threshold, int min_level,
                    int up_shift, int speech_shift, int down_shift, int warmup, int attack, int hang, int max_zc,
                    int window, int max_seg, hipStream_t stream);
int aiko_voice_activity(const float* audio, const int* state, int* state_out, int* level, int* zc, void* mask, int* seg,
                        int* count, int* speech, int* silent, int B, int F, int frame, int threshold, int min_level,
                        int up_shift, int speech_shift, int down_shift, int warmup, int attack, int hang, int max_zc,
                        int window, int max_seg, hipStream_t stream);
int aiko_spectrum_frames(const float* audio, const float* window, const float* twiddle, float* power, int B, long n,
                         int F, int n_fft, int hop, hipStream_t stream);
int aiko_spectrum_reduce(const float* power, const int* band_start, float* amplitudes, float* band_amplitudes,
                         int* peak_bins, float* peak_amplitudes, int* peak_counts, int B, int F, int n_fft, int bands,
                         int max_peaks, float inv_F, float lo, float hi, int k_lo, int k_hi, int local,
                         hipStream_t stream);
int aiko_spectrum(const float* audio, const float* window, const float* twiddle, const int* band_start, float* power,
                  float* amplitudes, float* band_amplitudes, int* peak_bins, float* peak_amplitudes, int* peak_counts,
                  int B, long n, int F, int n_fft, int hop, int bands, int max_peaks, float inv_F, float lo, float hi,
                  int k_lo, int k_hi, int local, hipStream_t stream);
int aiko_spectrum_graph(const int* peak_bins, const float* peak_amplitudes, const int* peak_counts, const int* bin_px,
                        void* image, int B, int H, int W, int K, int max_peaks, double y_max, int r, int g, int b,
                        hipStream_t stream);
int aiko_logmel(const float* audio, int B, int N, const float* mel, int n_mels, const int* mel_range,
                int n_fft, int hop, int F, float* logmel, int* gmax, void* dst, int rows, int pad, int ld,
                hipStream_t stream);
int aiko_window_shift(const float* src, const float* chunk, float* dst, int B, int W, int n, hipStream_t stream);

// ---- gemm_fp8.hip / linear_splitk.hip / attention.hip: the encoder's GEMMs and attention
int aiko_gemm_fp8(const void* a, const void* b, const float* sa, const float* sb, const float* bias,
                  const void* res, void* y, int M, int N, int K, int lda, int ldy, int ldr, int act,
                  int bm, int bn, int variant, const void* zero, const void* amx, int mxr, void* yq, void* ysc, int ldq, int ysr,
                  hipStream_t stream);
int aiko_rownorm_quant(const void* x, int ldx, const float* gamma, const float* beta, float eps,
                       void* yb, int ldyb, void* q, int ldq, float* qs, int M, int D, hipStream_t stream);
int aiko_linear_splitk(const void* x, const void* w, const float* bias, float* part, void* y, int M, int N, int K,
                       int ldx, int ldw, int ldy, int S, hipStream_t stream);
int aiko_attn_fwd(const void* q, const void* k, const void* v, void* o, int ldq, int ldk, int ldv,
                  int ldo, int B, int H, int T, int Tpad, int dh, float scale, void* work, long work_bytes,
                  void* oq, void* osc, int ldoq, int osr, hipStream_t stream);

// ---- decode_ops.hip: the decoder's step
int aiko_embed_tokens(const int* ids, const int* pos, const void* tok, const void* pemb, void* x, int B,
                      int d, int ldx, int vocab, int n_pos, hipStream_t stream);
int aiko_attn_decode(const void* q, int ldq, void* k, void* v, int ldk, int ldv, int S, const int* pos,
                     int T, const void* knew, const void* vnew, int ldnew, void* o, int ldo, int B,
                     int H, float scale, float* work, long work_elems, hipStream_t stream);
long aiko_attn_decode_work(int B, int H, int maxlen);
int aiko_dec_linear(const void* x, int ldx, const float* gamma, const float* beta, float eps, const void* w,
                    const float* sw, const float* bias, const void* res, int ldr, void* y, int ldy, int M, int N,
                    int K, int act, hipStream_t stream);
int aiko_argmax_step(const void* logits, int ld, int V, int B, int* ids, int* pos, int* out_tokens,
                     int max_len, const int* forced, int n_forced, int eot, int* done, unsigned* counter,
                     hipStream_t stream);

}  // extern "C"
