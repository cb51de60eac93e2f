// Torch operator registrations for the aiko_services_amd native library (torch.ops.aiko.*).
//
// Kernels live in csrc/kernels/*.hip behind plain extern "C" launchers (no torch headers in
// device code); this file validates shapes/dtypes/devices on the host — failing loudly, never
// falling back — and launches on the caller's current HIP stream so every op is capturable in
// a hipGraph (no allocation, no synchronisation inside a launch).
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <vector>

#include "kernels/conv_launch.h"

extern "C" {
int aiko_conv_igemm(const ConvLaunch* l);
int aiko_conv_glds(const ConvLaunch* l, const void* zero);
int aiko_conv_buf(const ConvLaunch* l, int occ, int mf32);
int aiko_conv_persist(const ConvLaunch* l);
int aiko_conv_wide(const ConvLaunch* l, int occ);
int aiko_conv_pw(const void* x, const void* w, const float* bias, const void* res, void* y, int M, int N,
                 int K, int ldx, int ldy, int ldr, int act, int cus, int mode, hipStream_t stream);
int aiko_conv_pw_dual(const void* x, const void* x2, const void* w, const float* bias, void* y, int M, int N,
                      int ldx, int ldx2, int ldy, int act, int Ho, int Wo, int H2, int W2, int s2, int cus,
                      hipStream_t stream);
int aiko_conv_glds_tail(const void* x, const void* w, const float* bias, int H, int W, int C, int Cc, int R, int S,
                        int stride, int pad, int Ho, int Wo, int M, int K, int N, int act, const void* w2, const float* b2,
                        void* y2, int ldy2, int ldw2, int act2, const void* zero, const int* dec, void* boxes,
                        float* scores, int* cls, hipStream_t stream);
int aiko_preprocess(const void* in, void* out, int B, int Hin, int Win, int Ho, int Wo, int Hp,
                    int Wp, int pad_t, int pad_l, int Hc, int Wc, int off_t, int off_l, float fill,
                    const float* mean, const float* std, int bgr, hipStream_t stream);
int aiko_stem_direct(const void* in, void* out, const void* w, const float* bias, int B, int Hin, int Win,
                     int Ho, int Wo, int Hc, int Wc, int off_t, int off_l, float fill, const float* mean,
                     const float* std, int bgr, int H1, int W1, int Cout, int ldo, int k, int stride, int pad,
                     int act, hipStream_t stream);
int aiko_conv3x3_rows(const void* x, const void* wimg, const float* bias, const void* res, void* y, int B, int H,
                      int W, int ldx, int ldy, int ldr, int act, int grid, hipStream_t stream);
int aiko_conv3x3_patchw(const void* x, const void* wimg, const float* bias, void* y, int B, int H, int W, int ldx,
                        int ldy, int act, int grid, hipStream_t stream);
int aiko_conv3x3_patch(const void* x, const void* wimg, const float* bias, void* y, int B, int H, int W, int ldy,
                       int act, int grid, hipStream_t stream);
int aiko_bneck_fused(const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                     const void* w3, const float* b3, void* y, int B, int H, int W, int cin, int grid,
                     unsigned* dbg, hipStream_t stream);
int aiko_conv3x3_exp(const void* t1, const void* w2, const float* b2, const void* w3img, const float* b3,
                     const void* res, void* y, int B, int H, int W, int N, int grid, hipStream_t stream);
int aiko_conv_chain(const void* A, const void* W1, const float* b1, const void* R, void* Y, const void* W2,
                    const float* b2, void* Z, const void* A2, int M, int K1, int N1, int N2, int grid,
                    hipStream_t stream);
int aiko_maxpool(const void* x, void* y, int B, int H, int W, int C, int Ho, int Wo, int k,
                 int s, int p, int ldx, int ldy, hipStream_t stream);
int aiko_resize_u8(const void* in, void* out, int B, int Hin, int Win, int Ho, int Wo, hipStream_t stream);
int aiko_roi_crop_u8(const void* frames, const float* det, const int* count, void* crops, int* rois, int B, int H,
                     int W, int max_det, int K, int Ho, int Wo, float margin, hipStream_t stream);
int aiko_draw_detections(const void* frames, void* out, const float* det, const int* count, const int* labels,
                         const float* scores, const void* names, const void* font, const void* palette, int B, int H,
                         int W, int max_det, int K, int C, int L, int G, int gh, int gw, int P, int t, int s,
                         float margin, int show_score, hipStream_t stream);
int aiko_redact_detections(const void* frames, void* out, const float* det, const int* count, const int* labels,
                           const void* select, int B, int H, int W, int max_det, int K, int C, int mode, int block,
                           int fill_rgb, float margin, hipStream_t stream);
int aiko_yuv_to_rgb_u8(const void* raw, void* out, int B, int H, int W, int fmt, const float* coef, int half,
                       hipStream_t stream);
int aiko_rgb_to_yuv_u8(const void* rgb, void* out, int B, int H, int W, int fmt, const float* coef, int half,
                       hipStream_t stream);
int aiko_resample(const void* pcm, int is_f32, const float* hist, const float* filt, float* out, float* hist_out,
                  int B, long n_in, int C, int L, int M, int T, hipStream_t stream);
int aiko_track_detections(const float* det, const int* count, const float* boxes, const int* meta, const int* issued,
                          float* boxes_out, int* meta_out, int* issued_out, int* ids, int* hits, int* labels, int B,
                          int max_det, int K, int T, float thr, int max_age, float min_score, int class_aware,
                          int label_mod, hipStream_t stream);
int aiko_motion_detect(const void* frames, const int* bg, const int* seen, int* bg_out, int* seen_out, float* det,
                       int* count, void* mask, int* cells, int B, int H, int W, int cell, int threshold,
                       int learn_shift, int learn_moving, int warmup, int min_cells, int max_det, hipStream_t stream);
int aiko_marker_detect(const void* frames, float* det, int* count, int* corners, int* ids, int* cands, void* mask,
                       void* work, int B, int H, int W, int N, int cell, int contrast, int min_side, int max_cand,
                       int max_det, int passes, hipStream_t stream);
int aiko_voice_activity(const float* audio, const int* state, int* state_out, int* level, int* zc, void* mask, int* seg,
                        int* count, int* speech, int* silent, int B, int F, int frame, int threshold, int min_level,
                        int up_shift, int speech_shift, int down_shift, int warmup, int attack, int hang, int max_zc,
                        int window, int max_seg, hipStream_t stream);
int aiko_spectrum(const float* audio, const float* window, const float* twiddle, const int* band_start, float* power,
                  float* amplitudes, float* band_amplitudes, int* peak_bins, float* peak_amplitudes, int* peak_counts,
                  int B, long n, int F, int n_fft, int hop, int bands, int max_peaks, float inv_F, float lo, float hi,
                  int k_lo, int k_hi, int local, hipStream_t stream);
int aiko_spectrum_graph(const int* peak_bins, const float* peak_amplitudes, const int* peak_counts, const int* bin_px,
                        void* image, int B, int H, int W, int K, int max_peaks, double y_max, int r, int g, int b,
                        hipStream_t stream);
int aiko_jpeg_encode(const void* raw, const void* tables, int header_len, void* workspace, void* stream, int* nbytes,
                     int B, int H, int W, int fmt, long cap, int seg_cap, hipStream_t stream_);
int aiko_jpeg_decode(const void* data, const int* nbytes, const void* desc, int desc_rows, void* workspace, void* raw,
                     int* status, int B, int H, int W, int fmt, long cap, int max_int, hipStream_t stream_);
int aiko_batchnorm(const void* x, void* y, const float* scale, const float* shift, long P, int C, int ldx,
                   int ldy, int act, hipStream_t stream);
int aiko_upsample2x(const void* x, void* y, int B, int H, int W, int C, int ldx, int ldy,
                    hipStream_t stream);
int aiko_yolo_decode(const void* const* feats, const int* H, const int* W, const int* strides,
                     const int* ld, int nlev, int B, int nc, int reg_max, void* boxes,
                     float* scores, int* cls, hipStream_t stream);
int aiko_gemm_fp8(const void* a, const void* b, const float* sa, const float* sb, const float* bias,
                  const void* res, void* y, int M, int N, int K, int lda, int ldy, int ldr, int act,
                  int bm, int bn, int variant, const void* zero, const void* amx, int mxr, void* yq, void* ysc, int ldq, int ysr,
                  hipStream_t stream);
int aiko_rownorm_quant(const void* x, int ldx, const float* gamma, const float* beta, float eps,
                       void* yb, int ldyb, void* q, int ldq, float* qs, int M, int D, hipStream_t stream);
int aiko_c2f_fused(const void* x, int ldx, const void* w1, const float* b1, int k1, const void* wa, const float* ba,
                   int ka, const void* wb, const float* bb, int kb, const void* w2, const float* b2, int k2, void* y, int ldy,
                   int B, int H, int W, int CI, int C, int CO, int shortcut, int rb, const void* xu, int ldxu, int cu, hipStream_t stream);
int aiko_c2f_bneck(const void* x, int ldx, const void* wa, const float* ba, int ka, const void* wb, const float* bb,
                   int kb, void* y, int ldy, int B, int H, int W, int C, int shortcut, int rb, hipStream_t stream);
int aiko_linear_splitk(const void* x, const void* w, const float* bias, float* part, void* y, int M, int N, int K,
                       int ldx, int ldw, int ldy, int S, hipStream_t stream);
int aiko_attn_fwd(const void* q, const void* k, const void* v, void* o, int ldq, int ldk, int ldv,
                  int ldo, int B, int H, int T, int Tpad, int dh, float scale, void* work, long work_bytes,
                  void* oq, void* osc, int ldoq, int osr, hipStream_t stream);
int aiko_logmel(const float* audio, int B, int N, const float* mel, int n_mels, const int* mel_range,
                int n_fft, int hop, int F, float* logmel, int* gmax, void* dst, int rows, int pad, int ld,
                hipStream_t stream);
int aiko_topk_nms(const void* boxes, const float* scores, const int* cls, int B, int A,
                  int max_cand, int max_det, float conf, float iou, float max_wh, float gain,
                  float pad_l, float pad_t, float img_w, float img_h, float* det, int* count,
                  void* workspace, hipStream_t stream);
size_t aiko_topk_nms_workspace(int B);
int aiko_avgpool(const void* x, void* y, int B, int HW, int C, hipStream_t stream);
int aiko_mean_rows_f32(const void* x, float* y, int B, int T, int C, long ldb, hipStream_t stream);
int aiko_zero_border_rows(void* x, int B, int rows, int C, hipStream_t stream);
int aiko_sppf_pool(void* x, int B, int H, int W, int ld, int c, int k, hipStream_t stream);
int aiko_window_shift(const float* src, const float* chunk, float* dst, int B, int W, int n, hipStream_t stream);
int aiko_conv_narrow(const void* x, const void* w, const float* bias, const void* res, void* y, int H, int W, int C,
                     int Cc, int R, int S, int stride, int pad, int Ho, int Wo, int M, int Cout, int K, int act,
                     int ldy, int ldr, int th, int wreg, hipStream_t stream);
int aiko_stem_pool_u8(const void* frames, const void* w, const float* bias, void* y, int B, int Hi, int Wi,
                      int Ho, int Wo, int Hm, int Wm, int ldy, const float* mean255, int variant, hipStream_t stream);
int aiko_stem_pool(const void* x, const void* w, const float* bias, void* y, int B, int Hp, int Wp,
                   int Ho, int Wo, int Hm, int Wm, int ldy, int variant, hipStream_t stream);
int aiko_softmax_topk(const void* logits, float* prob, int* index, int B, int N, int k,
                      hipStream_t stream);
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
}

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_cuda(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "aiko: ", name, " must be a GPU tensor");
}

// elements addressable from t.data_ptr() to the end of its storage
int64_t avail_elems(const at::Tensor& t) {
  return (int64_t)(t.storage().nbytes() / t.element_size()) - t.storage_offset();
}

void check_launch(int rc, const char* what) {
  TORCH_CHECK(rc == 0, "aiko: launch of ", what, " failed: ",
              rc < 0 ? "unsupported configuration" : hipGetErrorString((hipError_t)rc));
}

// geom = [H, W, C, Cc, R, S, stride, pad, Ho, Wo, M, act, ldy, ldr, bm, bn,
//         K1, H2, W2, C2, stride2 (the optional second source x2), [variant]]
// variant: a ConvVariant (kernels/conv_launch.h; the table with every kernel's tiles is VARIANTS
// in ops/conv.py), 0 when absent.  CONV_GLDS needs ``zero`` (>= 16 B of zeros on the device) as
// the source of conv padding.  An id without a case below is an error.
void conv_igemm_out(const at::Tensor& x, const c10::optional<at::Tensor>& x2, const at::Tensor& w,
                    const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& res,
                    at::Tensor& y, at::IntArrayRef geom, const c10::optional<at::Tensor>& zero) {
  TORCH_CHECK(geom.size() == 21 || geom.size() == 22, "aiko.conv_igemm_out: geom needs 21 or 22 ints");
  const int64_t variant = geom.size() == 22 ? geom[21] : 0;
  const int64_t H = geom[0], W = geom[1], C = geom[2], Cc = geom[3], R = geom[4], S = geom[5];
  const int64_t stride = geom[6], pad = geom[7], Ho = geom[8], Wo = geom[9], M = geom[10];
  const int64_t act = geom[11], ldy = geom[12], ldr = geom[13], bm = geom[14], bn = geom[15];
  const int64_t K1 = geom[16], H2 = geom[17], W2 = geom[18], C2 = geom[19], stride2 = geom[20];
  check_cuda(x, "x");
  check_cuda(w, "w");
  check_cuda(y, "y");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16 &&
                  y.scalar_type() == at::kBFloat16,
              "aiko.conv_igemm_out: x, w, y must be bfloat16");
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous(), "aiko.conv_igemm_out: w must be [Cout, K] contiguous");
  const int64_t Cout = w.size(0), K = w.size(1);
  const bool dual = x2.has_value() && x2->defined();
  const int64_t Kmain = dual ? K1 : K;
  TORCH_CHECK(Kmain >= R * S * Cc && Kmain % 64 == 0 && Kmain - R * S * Cc < 64, "aiko.conv_igemm_out: K=",
              Kmain, " must be R*S*Cc rounded up to a multiple of 64");
  const void* x2ptr = nullptr;
  if (dual) {
    check_cuda(*x2, "x2");
    TORCH_CHECK(x2->scalar_type() == at::kBFloat16, "aiko.conv_igemm_out: x2 must be bf16");
    TORCH_CHECK((K - K1) % 64 == 0 && K - K1 <= C2 && C2 % 8 == 0 && K1 > 0,
                "aiko.conv_igemm_out: second source needs K-K1 (multiple of 64) <= C2");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x2->data_ptr()) % 16 == 0, "aiko.conv_igemm_out: x2 alignment");
    TORCH_CHECK(M % (Ho * Wo) == 0 && (Ho - 1) * stride2 < H2 && (Wo - 1) * stride2 < W2 &&
                    avail_elems(*x2) >= (M / (Ho * Wo)) * H2 * W2 * C2,
                "aiko.conv_igemm_out: x2 too small for the output geometry");
    x2ptr = x2->data_ptr();
  }
  TORCH_CHECK(Cc % 8 == 0 && (Cc <= C || C == 4), "aiko.conv_igemm_out: Cc must be a multiple of 8 within the pixel pitch (or span pixels of a 4-channel stem input)");
  TORCH_CHECK(Cout % 8 == 0, "aiko.conv_igemm_out: Cout must be a multiple of 8");
  TORCH_CHECK(C % 8 == 0 || (C == 4 && Cc % 8 == 0), "aiko.conv_igemm_out: pixel pitch must keep 16-B alignment");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(y.data_ptr()) % 16 == 0,
              "aiko.conv_igemm_out: x and y must be 16-byte aligned");
  // x / y / residual may be channel-slice views (concat buffers): bound by storage extent
  const int64_t x_extent = avail_elems(x);
  TORCH_CHECK(x_extent < INT_MAX && w.numel() < INT_MAX, "aiko.conv_igemm_out: tensor too large for 32-bit offsets");
  TORCH_CHECK(ldy % 8 == 0 && ldy >= Cout, "aiko.conv_igemm_out: bad ldy");
  TORCH_CHECK(avail_elems(y) >= (M - 1) * ldy + Cout, "aiko.conv_igemm_out: y too small");
  const int64_t img_elems = H * W * C;
  // (the stem's 32-element chunks span pixels inside a row; its geometry keeps them in-row)
  const int64_t tail = Cc <= C ? Cc : C;
  TORCH_CHECK(M % (Ho * Wo) == 0 && x_extent >= (M / (Ho * Wo) - 1) * img_elems + (H * W - 1) * C + tail,
              "aiko.conv_igemm_out: x too small for M");
  const float* bptr = nullptr;
  if (bias.has_value() && bias->defined()) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == Cout && bias->is_contiguous(),
                "aiko.conv_igemm_out: bias must be fp32 [Cout]");
    bptr = bias->data_ptr<float>();
  }
  const void* rptr = nullptr;
  if (res.has_value() && res->defined()) {
    check_cuda(*res, "residual");
    TORCH_CHECK(res->scalar_type() == at::kBFloat16, "aiko.conv_igemm_out: residual must be bf16");
    TORCH_CHECK(ldr % 8 == 0 && avail_elems(*res) >= (M - 1) * ldr + Cout, "aiko.conv_igemm_out: bad residual");
    rptr = res->data_ptr();
  }
  ConvLaunch L;
  L.x = x.data_ptr(); L.w = w.data_ptr(); L.bias = bptr; L.res = rptr; L.y = y.data_ptr();
  L.H = H; L.W = W; L.C = C; L.Cc = Cc; L.R = R; L.S = S; L.stride = stride; L.pad = pad;
  L.Ho = Ho; L.Wo = Wo; L.M = M; L.Cout = Cout; L.K = K; L.act = act; L.ldy = ldy; L.ldr = ldr;
  L.bm = bm; L.bn = bn;
  L.x2 = x2ptr; L.K1 = K1; L.H2 = H2; L.W2 = W2; L.C2 = C2; L.stride2 = stride2;
  L.stream = cur_stream();
  // 64-channel K blocks inside one tap, byte offsets in 31 bits (the buffer-DMA kernels)
  const bool buf_shape = Cc % 64 == 0 && R * S <= 32 && x_extent * 2 < (1LL << 31) - 64 && w.numel() * 2 < (1LL << 31);
  const bool x2_fits = !dual || avail_elems(*x2) * 2 < (1LL << 31) - 64;
  int rc = -1;
  switch (variant) {
    case CONV_IGEMM:
      rc = aiko_conv_igemm(&L);
      break;
    case CONV_GLDS:
      TORCH_CHECK(zero.has_value() && zero->defined() && zero->is_cuda() && zero->nbytes() >= 16 &&
                      reinterpret_cast<uintptr_t>(zero->data_ptr()) % 16 == 0,
                  "aiko.conv_igemm_out: the LDS-DMA variant needs a zero page tensor (>= 16 B)");
      rc = aiko_conv_glds(&L, zero->data_ptr());
      break;
    case CONV_BUF:
    case CONV_BUF_OCC:
    case CONV_BUF_MF32:
    case CONV_BUF_WIDE4: {
      TORCH_CHECK(buf_shape, "aiko.conv_igemm_out: variant 2 needs Cc % 64 == 0, R*S <= 32 and operands < 2 GiB");
      TORCH_CHECK(x2_fits, "aiko.conv_igemm_out: x2 too large for variant 2");
      // occ: workgroups per CU forced by CONV_BUF_OCC (64x64: 5, else 3); 1 = the 4-wave wide tiles
      const int occ = variant == CONV_BUF_OCC ? (bm == 64 && bn == 64 ? 5 : 3) : variant == CONV_BUF_WIDE4 ? 1 : 0;
      rc = aiko_conv_buf(&L, occ, /*mf32=*/variant == CONV_BUF_MF32);
      break;
    }
    case CONV_PERSIST:
      TORCH_CHECK(buf_shape && K % 64 == 0,
                  "aiko.conv_igemm_out: variant 4 needs Cc % 64 == 0, R*S <= 32 and operands < 2 GiB");
      TORCH_CHECK(x2_fits, "aiko.conv_igemm_out: x2 too large for variant 4");
      rc = aiko_conv_persist(&L);
      break;
    case CONV_NARROW:
      TORCH_CHECK(!dual && ((R == 3 && S == 3 && pad == 1 && (stride == 1 || stride == 2)) ||
                            (R == 1 && S == 1 && pad == 0 && stride == 1)) &&
                      (Cc == 16 || Cc == 32) && (Cout == 16 || Cout == 32),
                  "aiko.conv_igemm_out: variant 7 needs a 3x3 / pad 1 / stride 1-2 or 1x1 / stride 1 conv with Cc, Cout in {16, 32}");
      // bm = output rows per workgroup (8 / 16); bn = 64: Cc-32 weights in registers
      rc = aiko_conv_narrow(L.x, L.w, bptr, rptr, L.y, H, W, C, Cc, R, S, stride, pad, Ho, Wo, M, Cout, K, act, ldy,
                            ldr, bm == 16 ? 16 : 8, bn == 64 ? 1 : 0, L.stream);
      break;
    case CONV_WIDE:
    case CONV_WIDE_OCC:
    case CONV_WIDE_DEEP:
    case CONV_WIDE_EXACT_N:
    case CONV_WIDE4_OCC:
    case CONV_WIDE_PERSIST:
      TORCH_CHECK(buf_shape, "aiko.conv_igemm_out: variant 8 needs Cc % 64 == 0, R*S <= 32 and operands < 2 GiB");
      TORCH_CHECK(x2_fits, "aiko.conv_igemm_out: x2 too large for variant 8");
      TORCH_CHECK(ldy % 8 == 0 && (!rptr || (ldr % 8 == 0 && reinterpret_cast<uintptr_t>(rptr) % 16 == 0)),
                  "aiko.conv_igemm_out: variant 8 needs 16-B aligned rows");
      // aiko_conv_wide's form: 1 = one workgroup per CU, 2 = several; the others go by their id
      rc = aiko_conv_wide(&L, variant == CONV_WIDE ? 1 : variant == CONV_WIDE_OCC ? 2 : (int)variant);
      break;
    case CONV_PW:
    case CONV_PW_RESIDENT:
    case CONV_PW_RESIDENT_AB: {
      static int cus = 0;
      if (cus == 0) {
        int dev = 0, n = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus = n;
      }
      if (variant == CONV_PW_RESIDENT && dual) {
        // fused projection on the resident-weight kernel: 1x1 main source of 128 channels + a
        // 1x1 / stride-s2 second source of 256 channels
        TORCH_CHECK(R == 1 && S == 1 && stride == 1 && pad == 0 && Cc == 128 && K1 == 128 && K == 384 &&
                        Cout % 128 == 0 && C % 8 == 0 && !rptr && x_extent * 2 < (1LL << 31) - 64 && x2_fits &&
                        avail_elems(y) * 2 < (1LL << 31) && ldy % 8 == 0,
                    "aiko.conv_igemm_out: variant 13 with a second source needs a 128 + 256 column 1x1 projection, "
                    "Cout % 128 == 0, no residual and operands < 2 GiB");
        TORCH_CHECK(!bptr || reinterpret_cast<uintptr_t>(bptr) % 16 == 0, "aiko.conv_igemm_out: bias alignment");
        rc = aiko_conv_pw_dual(L.x, x2ptr, L.w, bptr, L.y, M, Cout, C, C2, ldy, act, Ho, Wo, H2, W2, stride2, cus,
                               L.stream);
        break;
      }
      // 1x1 / stride 1 / one source, x rows = pixels at pitch C
      const bool pw_shape = variant == CONV_PW ? (K % 256 == 0 && Cout % 128 == 0)
                                               : ((K == 128 && Cout % 256 == 0) || (K == 256 && Cout % 128 == 0) ||
                                                  (K == 512 && Cout % 64 == 0));
      TORCH_CHECK(!dual && R == 1 && S == 1 && stride == 1 && pad == 0 && Cc == K && pw_shape &&
                      C % 8 == 0 && x_extent * 2 < (1LL << 31) - 64 && w.numel() * 2 < (1LL << 31) &&
                      avail_elems(y) * 2 < (1LL << 31),
                  "aiko.conv_igemm_out: variants 12/13 need a 1x1/s1 single-source conv with K % 256 == 0 "
                  "(13: K = 128 / 256 / 512), Cout a multiple of the channel block and operands < 2 GiB");
      TORCH_CHECK(ldy % 8 == 0 && (!rptr || (ldr % 8 == 0 && reinterpret_cast<uintptr_t>(rptr) % 16 == 0 &&
                                            avail_elems(*res) * 2 < (1LL << 31) - 64)),
                  "aiko.conv_igemm_out: variant 12 needs 16-B aligned rows");
      TORCH_CHECK(!bptr || reinterpret_cast<uintptr_t>(bptr) % 16 == 0, "aiko.conv_igemm_out: bias alignment");
      // mode: 0 streamed weights, 1 resident weight block, 2 resident with the residual at its own tile
      rc = aiko_conv_pw(L.x, L.w, bptr, rptr, L.y, M, Cout, K, C, ldy, ldr, act, cus,
                        variant == CONV_PW_RESIDENT ? 1 : variant == CONV_PW_RESIDENT_AB ? 2 : 0, L.stream);
      break;
    }
    default:   // CONV_PATCH / PATCHW / ROWS have operators of their own
      TORCH_CHECK(false, "aiko.conv_igemm_out: unknown variant ", variant);
  }
  check_launch(rc, "conv_igemm");
}

// canvas = [Hc, Wc, off_t, off_l, fill]: the frame is resized to (Ho, Wo) and placed at
// (off_t, off_l) inside an Hc x Wc canvas of colour ``fill`` at (pad_t, pad_l) of ``out``.
void preprocess_out(const at::Tensor& frames, at::Tensor& out, int64_t Ho, int64_t Wo,
                    int64_t pad_t, int64_t pad_l, at::ArrayRef<double> mean,
                    at::ArrayRef<double> std, bool bgr, at::ArrayRef<double> canvas) {
  check_cuda(frames, "frames");
  check_cuda(out, "out");
  TORCH_CHECK(frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3 &&
                  frames.is_contiguous(),
              "aiko.preprocess_out: frames must be uint8 [B, H, W, 3] contiguous");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 && out.dim() == 4 && out.size(3) == 4 &&
                  out.is_contiguous() && out.size(0) == frames.size(0),
              "aiko.preprocess_out: out must be bf16 [B, Hp, Wp, 4] contiguous");
  TORCH_CHECK(mean.size() == 3 && std.size() == 3, "aiko.preprocess_out: mean/std need 3 values");
  int64_t Hc = Ho, Wc = Wo, off_t = 0, off_l = 0;
  double fill = 0.0;
  if (!canvas.empty()) {
    TORCH_CHECK(canvas.size() == 5, "aiko.preprocess_out: canvas = [Hc, Wc, off_t, off_l, fill]");
    Hc = (int64_t)canvas[0]; Wc = (int64_t)canvas[1];
    off_t = (int64_t)canvas[2]; off_l = (int64_t)canvas[3]; fill = canvas[4];
  }
  TORCH_CHECK(off_t >= 0 && off_l >= 0 && off_t + Ho <= Hc && off_l + Wo <= Wc,
              "aiko.preprocess_out: image must lie inside the canvas");
  TORCH_CHECK(pad_t + Hc <= out.size(1) && pad_l + Wc <= out.size(2), "aiko.preprocess_out: out too small");
  float m[3] = {(float)mean[0], (float)mean[1], (float)mean[2]};
  float s[3] = {(float)std[0], (float)std[1], (float)std[2]};
  const int rc = aiko_preprocess(frames.data_ptr(), out.data_ptr(), frames.size(0), frames.size(1),
                                 frames.size(2), Ho, Wo, out.size(1), out.size(2), pad_t, pad_l,
                                 Hc, Wc, off_t, off_l, (float)fill, m, s, bgr ? 1 : 0, cur_stream());
  check_launch(rc, "preprocess");
}

int64_t pixel_pitch(const at::Tensor& t, const char* op);

// 3x3 / stride 1 / pad 1 conv, 64 -> 64 channels, with an LDS-resident input patch (conv_patch.hip).
// x [B, H, W, 64] contiguous; wimg the [9, 2, 4, 64, 8] fragment image (ops.conv.patch_weight);
// y [B, H, W, >= 64] NHWC with unit channel stride (a channel slice of a wider buffer is fine).
void conv3x3_patch_out(const at::Tensor& x, const at::Tensor& wimg, const c10::optional<at::Tensor>& bias,
                       at::Tensor& y, int64_t act, int64_t grid) {
  check_cuda(x, "x");
  check_cuda(wimg, "wimg");
  check_cuda(y, "y");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && wimg.scalar_type() == at::kBFloat16 && y.scalar_type() == at::kBFloat16,
              "aiko.conv3x3_patch_out: bf16 tensors");
  TORCH_CHECK(x.dim() == 4 && x.size(3) == 64 && x.is_contiguous(), "aiko.conv3x3_patch_out: x must be [B, H, W, 64] contiguous");
  TORCH_CHECK(wimg.is_contiguous() && wimg.numel() == 9 * 64 * 64, "aiko.conv3x3_patch_out: wimg must be the 36864-element image");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2);
  TORCH_CHECK(W + 8 <= 64, "aiko.conv3x3_patch_out: W <= 56");
  TORCH_CHECK(y.dim() == 4 && y.size(0) == B && y.size(1) == H && y.size(2) == W && y.size(3) == 64 && y.stride(3) == 1 &&
                  y.stride(2) % 8 == 0 && y.stride(1) == W * y.stride(2) && y.stride(0) == H * W * y.stride(2) &&
                  reinterpret_cast<uintptr_t>(y.data_ptr()) % 16 == 0,
              "aiko.conv3x3_patch_out: y must be [B, H, W, 64] NHWC (16-B aligned pixel pitch)");
  TORCH_CHECK(x.numel() * 2 < (1LL << 31) - 64 && avail_elems(y) * 2 < (1LL << 31) - 64,
              "aiko.conv3x3_patch_out: tensors too large for 32-bit offsets");
  TORCH_CHECK(act == 0 || act == 1 || act == 2, "aiko.conv3x3_patch_out: act none / relu / silu");
  const float* bptr = nullptr;
  if (bias.has_value() && bias->defined()) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == 64, "aiko.conv3x3_patch_out: bias fp32 [64]");
    bptr = bias->data_ptr<float>();
  }
  check_launch(aiko_conv3x3_patch(x.data_ptr(), wimg.data_ptr(), bptr, y.data_ptr(), (int)B, (int)H, (int)W,
                                  (int)y.stride(2), (int)act, (int)grid, cur_stream()),
               "conv3x3_patch");
}

// 3x3 / stride 1 / pad 1 conv, 128 -> 128 channels, W = 28, patch per 14-row tile with streamed
// weights (conv_patchw.hip).  x [B, H, 28, >= 128] NHWC (16-B aligned pixel pitch); wimg the
// [4, 9, 8, 64, 8] fragment image (ops.conv.patchw_weight); y [B, H, 28, >= 128] NHWC.
void conv3x3_patchw_out(const at::Tensor& x, const at::Tensor& wimg, const c10::optional<at::Tensor>& bias,
                        at::Tensor& y, int64_t act, int64_t grid) {
  check_cuda(x, "x");
  check_cuda(wimg, "wimg");
  check_cuda(y, "y");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && wimg.scalar_type() == at::kBFloat16 && y.scalar_type() == at::kBFloat16,
              "aiko.conv3x3_patchw_out: bf16 tensors");
  TORCH_CHECK(x.dim() == 4 && x.size(3) >= 128 && x.size(2) == 28 && x.stride(3) == 1 && x.stride(2) % 8 == 0 &&
                  x.stride(1) == 28 * x.stride(2) && x.stride(0) == x.size(1) * x.stride(1) &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "aiko.conv3x3_patchw_out: x must be [B, H, 28, >= 128] NHWC with a 16-B aligned pixel pitch");
  TORCH_CHECK(wimg.is_contiguous() && wimg.numel() == 9 * 128 * 128, "aiko.conv3x3_patchw_out: wimg must be the 147456-element image");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2);
  TORCH_CHECK(y.dim() == 4 && y.size(0) == B && y.size(1) == H && y.size(2) == W && y.size(3) == 128 && y.stride(3) == 1 &&
                  y.stride(2) % 8 == 0 && y.stride(1) == W * y.stride(2) && y.stride(0) == H * W * y.stride(2) &&
                  reinterpret_cast<uintptr_t>(y.data_ptr()) % 16 == 0,
              "aiko.conv3x3_patchw_out: y must be [B, H, 28, 128] NHWC (16-B aligned pixel pitch)");
  TORCH_CHECK(avail_elems(x) * 2 < (1LL << 31) - 64 && avail_elems(y) * 2 < (1LL << 31) - 64,
              "aiko.conv3x3_patchw_out: tensors too large for 32-bit offsets");
  TORCH_CHECK(act == 0 || act == 1, "aiko.conv3x3_patchw_out: act none / relu");
  const float* bptr = nullptr;
  if (bias.has_value() && bias->defined()) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == 128, "aiko.conv3x3_patchw_out: bias fp32 [128]");
    bptr = bias->data_ptr<float>();
  }
  check_launch(aiko_conv3x3_patchw(x.data_ptr(), wimg.data_ptr(), bptr, y.data_ptr(), (int)B, (int)H, (int)W,
                                   (int)x.stride(2), (int)y.stride(2), (int)act, (int)grid, cur_stream()),
               "conv3x3_patchw");
}

// 3x3 / stride 1 / pad 1 conv, 32 -> 32 channels, W = 80, as a persistent row stream
// (conv_rows.hip).  x / res / y: [B, H, 80, >= 32] NHWC views whose rows are uniformly strided
// (channel slices of wider buffers are fine); wimg the [9, 2, 64, 8] fragment image
// (ops.conv.rows_weight).  act bits 0-3: none / ReLU / SiLU, bit 4: residual after the activation.
void conv3x3_rows_out(const at::Tensor& x, const at::Tensor& wimg, const c10::optional<at::Tensor>& bias,
                      const c10::optional<at::Tensor>& res, at::Tensor& y, int64_t act, int64_t grid) {
  check_cuda(x, "x");
  check_cuda(wimg, "wimg");
  check_cuda(y, "y");
  auto rows_ok = [](const at::Tensor& t, int64_t B, int64_t H) {
    return t.dim() == 4 && t.size(0) == B && t.size(1) == H && t.size(2) == 80 && t.size(3) >= 32 && t.stride(3) == 1 &&
           t.stride(2) % 8 == 0 && t.stride(1) == 80 * t.stride(2) && t.stride(0) == H * t.stride(1) &&
           reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 && t.scalar_type() == at::kBFloat16 &&
           avail_elems(t) * 2 < (1LL << 31) - 64;
  };
  const int64_t B = x.size(0), H = x.size(1);
  TORCH_CHECK(rows_ok(x, B, H), "aiko.conv3x3_rows_out: x must be [B, H, 80, >= 32] bf16 with uniformly strided rows");
  TORCH_CHECK(rows_ok(y, B, H) && y.size(3) == 32, "aiko.conv3x3_rows_out: y must be [B, H, 80, 32] bf16 (a slice is fine)");
  TORCH_CHECK(wimg.is_contiguous() && wimg.numel() == 9 * 32 * 32 && wimg.scalar_type() == at::kBFloat16,
              "aiko.conv3x3_rows_out: wimg must be the 9216-element bf16 image");
  const void* rptr = nullptr;
  int64_t ldr = 0;
  if (res.has_value() && res->defined()) {
    check_cuda(*res, "res");
    TORCH_CHECK(rows_ok(*res, B, H), "aiko.conv3x3_rows_out: res must be [B, H, 80, >= 32] bf16 with uniformly strided rows");
    rptr = res->data_ptr();
    ldr = res->stride(2);
  }
  TORCH_CHECK((act & 15) <= 2 && (act & ~31) == 0, "aiko.conv3x3_rows_out: act none / relu / silu (+16: residual after)");
  const float* bptr = nullptr;
  if (bias.has_value() && bias->defined()) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == 32, "aiko.conv3x3_rows_out: bias fp32 [32]");
    bptr = bias->data_ptr<float>();
  }
  check_launch(aiko_conv3x3_rows(x.data_ptr(), wimg.data_ptr(), bptr, rptr, y.data_ptr(), (int)B, (int)H, 80,
                                 (int)x.stride(2), (int)y.stride(2), (int)ldr, (int)act, (int)grid, cur_stream()),
               "conv3x3_rows");
}

// Chained 1x1 convs at a bottleneck boundary (conv_chain.hip):
//   Y = relu(A W1^T + b1 + R) [M, N1],  Z = relu(Y W2^T + b2) [M, N2]
//   (K1, N1, N2) in {(64, 256, 64), (64, 256, 128), (128, 512, 128), (128, 512, 256)}
void conv_chain_out(const at::Tensor& A, const at::Tensor& W1, const at::Tensor& b1, const c10::optional<at::Tensor>& R_opt,
                    at::Tensor& Y, const at::Tensor& W2, const at::Tensor& b2, at::Tensor& Z, int64_t grid,
                    const c10::optional<at::Tensor>& A2_opt) {
  const bool dual = A2_opt.has_value() && A2_opt->defined();
  TORCH_CHECK(dual != (R_opt.has_value() && R_opt->defined()),
              "aiko.conv_chain_out: exactly one of R (identity residual) and A2 (fused projection shortcut)");
  const at::Tensor& R = dual ? *A2_opt : *R_opt;   // (validated by the dual branch below when dual)
  for (const at::Tensor* t : {&A, &W1, &b1, &R, (const at::Tensor*)&Y, &W2, &b2, (const at::Tensor*)&Z}) {
    check_cuda(*t, "conv_chain operand");
    TORCH_CHECK(t->is_contiguous() && reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "aiko.conv_chain_out: operands must be contiguous and 16-byte aligned");
  }
  for (const at::Tensor* t : {&A, &W1, &R, (const at::Tensor*)&Y, &W2, (const at::Tensor*)&Z})
    TORCH_CHECK(t->scalar_type() == at::kBFloat16, "aiko.conv_chain_out: bf16 activations / weights");
  TORCH_CHECK(b1.scalar_type() == at::kFloat && b2.scalar_type() == at::kFloat, "aiko.conv_chain_out: fp32 biases");
  TORCH_CHECK(W1.dim() == 2 && W2.dim() == 2, "aiko.conv_chain_out: W1 / W2 [Cout, K]");
  const int64_t N1 = W1.size(0), K1 = W1.size(1), N2 = W2.size(0);
  const bool shape_ok = dual ? (K1 == 128 && N1 == 256 && N2 == 64)
                             : ((K1 == 64 && N1 == 256 && (N2 == 64 || N2 == 128)) ||
                                (K1 == 128 && N1 == 512 && (N2 == 128 || N2 == 256)) ||
                                (K1 == 256 && N1 == 1024 && N2 == 256));
  TORCH_CHECK(shape_ok, "aiko.conv_chain_out: unsupported (K1, N1, N2) = (", K1, ", ", N1, ", ", N2, ")", dual ? " dual" : "");
  const int64_t ka = dual ? K1 / 2 : K1;           // width of each A source
  const int64_t M = A.numel() / ka;
  TORCH_CHECK(A.size(-1) == ka && b1.numel() == N1 && W2.size(1) == N1 && b2.numel() == N2,
              "aiko.conv_chain_out: A [.., K1 (or K1/2 per source)], b1 [N1], W2 [N2, N1], b2 [N2]");
  if (dual) {
    TORCH_CHECK(R.numel() == M * ka && R.size(-1) == ka, "aiko.conv_chain_out: A2 [M, K1/2]");
  } else {
    TORCH_CHECK(R.numel() == M * N1 && R.size(-1) == N1, "aiko.conv_chain_out: R [M, N1]");
  }
  TORCH_CHECK(Y.numel() == M * N1 && Y.size(-1) == N1 && Z.numel() == M * N2 && Z.size(-1) == N2,
              "aiko.conv_chain_out: Y [M, N1], Z [M, N2]");
  TORCH_CHECK(M % 64 == 0, "aiko.conv_chain_out: M must be a multiple of 64");
  check_launch(aiko_conv_chain(A.data_ptr(), W1.data_ptr(), b1.data_ptr<float>(), dual ? nullptr : R.data_ptr(),
                               Y.data_ptr(), W2.data_ptr(), b2.data_ptr<float>(), Z.data_ptr(),
                               dual ? R.data_ptr() : nullptr, M, K1, N1, N2, grid, cur_stream()),
               "conv_chain");
}

// A YOLOv8 C2f block with one bottleneck in one launch (c2f_fused.hip): x [B, H, W, >= CI] ->
// y [B, H, W, >= CO]; weights / biases as the four ConvSpecs hold them (cv1, conv a, conv b, cv2:
// [Cout, K padded] bf16 + fp32 biases, SiLU everywhere).  Shapes without an instantiation fail.
void c2f_fused_out(const at::Tensor& x, const at::Tensor& w1, const at::Tensor& b1, const at::Tensor& wa,
                   const at::Tensor& ba, const at::Tensor& wb, const at::Tensor& bb, const at::Tensor& w2,
                   const at::Tensor& b2, at::Tensor& y, int64_t ci, bool shortcut, int64_t rb,
                   const c10::optional<at::Tensor>& xu_opt) {
  for (const at::Tensor* t : {&x, &w1, &b1, &wa, &ba, &wb, &bb, &w2, &b2, (const at::Tensor*)&y}) check_cuda(*t, "c2f operand");
  for (const at::Tensor* t : {&x, &w1, &wa, &wb, &w2, (const at::Tensor*)&y})
    TORCH_CHECK(t->scalar_type() == at::kBFloat16, "aiko.c2f_fused_out: bf16 activations / weights");
  for (const at::Tensor* t : {&b1, &ba, &bb, &b2})
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous(), "aiko.c2f_fused_out: fp32 contiguous biases");
  for (const at::Tensor* t : {&w1, &wa, &wb, &w2})
    TORCH_CHECK(t->dim() == 2 && t->is_contiguous() && t->size(1) % 8 == 0, "aiko.c2f_fused_out: weights [Cout, K] contiguous");
  TORCH_CHECK(x.dim() == 4 && y.dim() == 4 && x.size(0) == y.size(0) && x.size(1) == y.size(1) && x.size(2) == y.size(2),
              "aiko.c2f_fused_out: x, y [B, H, W, C]");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2);
  const int64_t C = wa.size(0), CO = w2.size(0), CI = ci;
  TORCH_CHECK(CI % 32 == 0 && w1.size(1) >= CI, "aiko.c2f_fused_out: cv1 K (input channels) a multiple of 32");
  TORCH_CHECK(w1.size(0) == 2 * C && wb.size(0) == C && wa.size(1) >= 9 * C && wb.size(1) >= 9 * C &&
                  ((9 * C + 31) / 32) * 32 <= wa.size(1) && ((9 * C + 31) / 32) * 32 <= wb.size(1) && w2.size(1) >= 3 * C &&
                  b1.numel() == 2 * C && ba.numel() == C && bb.numel() == C && b2.numel() == CO,
              "aiko.c2f_fused_out: inconsistent cv1 / bottleneck / cv2 shapes");
  const int64_t ldx = x.stride(2), ldy = y.stride(2);
  TORCH_CHECK(x.stride(3) == 1 && y.stride(3) == 1 && x.stride(2) == ldx && y.stride(2) == ldy &&
                  x.stride(1) == W * ldx && y.stride(1) == W * ldy && x.stride(0) == H * W * ldx &&
                  y.stride(0) == H * W * ldy && ldx % 8 == 0 && ldy % 4 == 0 && x.size(3) >= CI && y.size(3) >= CO &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(y.data_ptr()) % 8 == 0,
              "aiko.c2f_fused_out: NHWC views with 16-B aligned pixels");
  // optional in-place 2x upsample source for input channels [0, cu): xu [B, H/2, W/2, cu] (NHWC view)
  const void* xup = nullptr;
  int64_t ldxu = 0, cu = 0;
  if (xu_opt.has_value() && xu_opt->defined()) {
    const at::Tensor& xu = *xu_opt;
    check_cuda(xu, "c2f upsample source");
    TORCH_CHECK(xu.scalar_type() == at::kBFloat16 && xu.dim() == 4 && xu.size(0) == B && 2 * xu.size(1) == H &&
                    2 * xu.size(2) == W && xu.stride(3) == 1 && xu.stride(1) == xu.size(2) * xu.stride(2) &&
                    xu.stride(0) == xu.size(1) * xu.stride(1) && xu.stride(2) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(xu.data_ptr()) % 16 == 0,
                "aiko.c2f_fused_out: xu must be an NHWC [B, H/2, W/2, cu] view with 16-B aligned pixels");
    cu = xu.size(3);
    TORCH_CHECK(cu % 32 == 0 && cu < CI, "aiko.c2f_fused_out: xu channels a multiple of 32 below ci");
    xup = xu.data_ptr();
    ldxu = xu.stride(2);
  }
  check_launch(aiko_c2f_fused(x.data_ptr(), (int)ldx, w1.data_ptr(), b1.data_ptr<float>(), (int)w1.size(1), wa.data_ptr(),
                              ba.data_ptr<float>(), (int)wa.size(1), wb.data_ptr(), bb.data_ptr<float>(), (int)wb.size(1),
                              w2.data_ptr(), b2.data_ptr<float>(), (int)w2.size(1), y.data_ptr(), (int)ldy, (int)B, (int)H,
                              (int)W, (int)CI, (int)C, (int)CO, shortcut ? 1 : 0, (int)rb, xup, (int)ldxu, (int)cu,
                              cur_stream()),
               "c2f_fused");
}


// One YOLOv8 C2f bottleneck (3x3 C -> C twice + shortcut) in one launch (c2f_fused.hip):
// x = s, y = c as NHWC channel-slice views of the C2f's concat buffer.
void c2f_bneck_out(const at::Tensor& x, const at::Tensor& wa, const at::Tensor& ba, const at::Tensor& wb,
                   const at::Tensor& bb, at::Tensor& y, bool shortcut, int64_t rb) {
  for (const at::Tensor* t : {&x, &wa, &ba, &wb, &bb, (const at::Tensor*)&y}) check_cuda(*t, "c2f bottleneck operand");
  for (const at::Tensor* t : {&x, &wa, &wb, (const at::Tensor*)&y})
    TORCH_CHECK(t->scalar_type() == at::kBFloat16, "aiko.c2f_bneck_out: bf16 activations / weights");
  TORCH_CHECK(ba.scalar_type() == at::kFloat && bb.scalar_type() == at::kFloat && ba.is_contiguous() && bb.is_contiguous(),
              "aiko.c2f_bneck_out: fp32 biases");
  const int64_t C = wa.size(0);
  TORCH_CHECK(wa.dim() == 2 && wb.dim() == 2 && wa.is_contiguous() && wb.is_contiguous() && wb.size(0) == C &&
                  wa.size(1) >= 9 * C && wb.size(1) >= 9 * C && wa.size(1) % 8 == 0 && wb.size(1) % 8 == 0 &&
                  ba.numel() == C && bb.numel() == C,
              "aiko.c2f_bneck_out: 3x3 weights [C, >= 9C]");
  TORCH_CHECK(x.dim() == 4 && y.dim() == 4 && x.sizes() == y.sizes() && x.size(3) == C, "aiko.c2f_bneck_out: x, y [B, H, W, C]");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), ldx = x.stride(2), ldy = y.stride(2);
  TORCH_CHECK(x.stride(3) == 1 && y.stride(3) == 1 && x.stride(1) == W * ldx && y.stride(1) == W * ldy &&
                  x.stride(0) == H * W * ldx && y.stride(0) == H * W * ldy && ldx % 8 == 0 && ldy % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(y.data_ptr()) % 8 == 0,
              "aiko.c2f_bneck_out: NHWC channel-slice views, 16-B aligned pixels");
  check_launch(aiko_c2f_bneck(x.data_ptr(), (int)ldx, wa.data_ptr(), ba.data_ptr<float>(), (int)wa.size(1), wb.data_ptr(),
                              bb.data_ptr<float>(), (int)wb.size(1), y.data_ptr(), (int)ldy, (int)B, (int)H, (int)W, (int)C,
                              shortcut ? 1 : 0, (int)rb, cur_stream()),
               "c2f_bneck");
}

// R x R conv (Cout N = 64, 80 or 128, exact-N tile, LDS-DMA kernel) with a fused trailing 1x1 N -> N + bias
// (conv_glds.hip, TAIL): y2 = act2((act(conv(x) + bias)) . w2[:, :N]^T + b2).  x, y2: NHWC channel-slice
// views; w [N, K] and w2 [N, >= ceil32(N)] with zero K padding (conv spec layout).
void conv_glds_tail_out(const at::Tensor& x, const at::Tensor& w, const at::Tensor& bias, const at::Tensor& w2,
                        const at::Tensor& b2, at::Tensor& y2, int64_t R, int64_t stride, int64_t pad, int64_t act,
                        int64_t act2, const at::Tensor& zero) {
  TORCH_CHECK(act2 == 0 || act2 == 2, "aiko.conv_glds_tail_out: act2 = 0 (none) or 2 (SiLU)");
  for (const at::Tensor* t : {&x, &w, &bias, &w2, &b2, (const at::Tensor*)&y2, &zero}) check_cuda(*t, "conv tail operand");
  for (const at::Tensor* t : {&x, &w, &w2, (const at::Tensor*)&y2})
    TORCH_CHECK(t->scalar_type() == at::kBFloat16, "aiko.conv_glds_tail_out: bf16 activations / weights");
  const int64_t N = w.size(0);
  TORCH_CHECK(N == 64 || N == 80 || N == 128, "aiko.conv_glds_tail_out: N = 64, 80 or 128");
  TORCH_CHECK(bias.scalar_type() == at::kFloat && b2.scalar_type() == at::kFloat && bias.numel() == N &&
                  b2.numel() == N && bias.is_contiguous() && b2.is_contiguous(),
              "aiko.conv_glds_tail_out: fp32 biases [N]");
  TORCH_CHECK(x.dim() == 4 && y2.dim() == 4 && x.stride(3) == 1 && y2.stride(3) == 1, "aiko.conv_glds_tail_out: NHWC");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), Cc = x.size(3), C = x.stride(2);
  TORCH_CHECK(x.stride(1) == W * C && x.stride(0) == H * W * C && C % 8 == 0 && Cc % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "aiko.conv_glds_tail_out: x must be an NHWC (channel-slice) view with 16-B aligned pixels");
  const int64_t K = (R * R * Cc + 63) / 64 * 64;
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous() && w.size(1) == K,
              "aiko.conv_glds_tail_out: w must be [N, ceil64(R*R*Cc)]");
  TORCH_CHECK(w2.dim() == 2 && w2.is_contiguous() && w2.size(0) == N && w2.size(1) >= (N + 31) / 32 * 32 &&
                  w2.size(1) % 8 == 0,
              "aiko.conv_glds_tail_out: w2 must be [N, >= ceil32(N)] (zero past column N)");
  const int64_t Ho = (H + 2 * pad - R) / stride + 1, Wo = (W + 2 * pad - R) / stride + 1;
  const int64_t ldy2 = y2.stride(2);
  TORCH_CHECK(y2.size(0) == B && y2.size(1) == Ho && y2.size(2) == Wo && y2.size(3) == N &&
                  y2.stride(1) == Wo * ldy2 && y2.stride(0) == Ho * Wo * ldy2 && ldy2 % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(y2.data_ptr()) % 16 == 0,
              "aiko.conv_glds_tail_out: y2 must be an NHWC [B, Ho, Wo, N] (channel-slice) view");
  const int64_t M = B * Ho * Wo;
  TORCH_CHECK(avail_elems(x) < INT_MAX && avail_elems(y2) < INT_MAX, "aiko.conv_glds_tail_out: 32-bit offsets");
  check_launch(aiko_conv_glds_tail(x.data_ptr(), w.data_ptr(), bias.data_ptr<float>(), (int)H, (int)W, (int)C, (int)Cc,
                                   (int)R, (int)R, (int)stride, (int)pad, (int)Ho, (int)Wo, (int)M, (int)K, (int)N, (int)act,
                                   w2.data_ptr(), b2.data_ptr<float>(), y2.data_ptr(), (int)ldy2, (int)w2.size(1),
                                   (int)act2, zero.data_ptr(), nullptr, nullptr, nullptr, nullptr, cur_stream()),
               "conv_glds_tail");
}

// The detect head's box / class branch (R x R conv + 1x1 as above) with the YOLOv8 decode in the
// epilogue instead of a stored head output: mode 1 (N = 64, 4 x 16 DFL bins) writes xyxy boxes
// [B, A] float4 at anchors astart + h * W + w, mode 2 (N = 80) sigmoid(max logit over the first nc)
// and its class into scores / cls [B, A] (ops.detect.yolo_decode semantics, bf16-rounded inputs).
void conv_glds_tail_decode_out(const at::Tensor& x, const at::Tensor& w, const at::Tensor& bias, const at::Tensor& w2,
                               const at::Tensor& b2, at::Tensor& boxes, at::Tensor& scores, at::Tensor& cls, int64_t R,
                               int64_t pad, int64_t act, int64_t mode, int64_t nc, int64_t level_stride, int64_t astart,
                               const at::Tensor& zero) {
  for (const at::Tensor* t : {&x, &w, &bias, &w2, &b2, (const at::Tensor*)&boxes, (const at::Tensor*)&scores,
                              (const at::Tensor*)&cls, &zero})
    check_cuda(*t, "conv tail decode operand");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16 && w2.scalar_type() == at::kBFloat16,
              "aiko.conv_glds_tail_decode_out: bf16 activations / weights");
  TORCH_CHECK(bias.scalar_type() == at::kFloat && b2.scalar_type() == at::kFloat && bias.is_contiguous() && b2.is_contiguous(),
              "aiko.conv_glds_tail_decode_out: fp32 biases");
  const int64_t N = w.size(0);
  TORCH_CHECK((mode == 1 && N == 64) || (mode == 2 && N == 80), "aiko.conv_glds_tail_decode_out: mode 1 needs N = 64, mode 2 N = 80");
  TORCH_CHECK(bias.numel() == N && b2.numel() == N && nc >= 1 && nc <= N, "aiko.conv_glds_tail_decode_out: biases [N], 1 <= nc <= N");
  TORCH_CHECK(x.dim() == 4 && x.stride(3) == 1, "aiko.conv_glds_tail_decode_out: NHWC x");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), Cc = x.size(3), C = x.stride(2);
  TORCH_CHECK(x.stride(1) == W * C && x.stride(0) == H * W * C && C % 8 == 0 && Cc % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "aiko.conv_glds_tail_decode_out: x must be an NHWC (channel-slice) view with 16-B aligned pixels");
  const int64_t K = (R * R * Cc + 63) / 64 * 64;
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous() && w.size(1) == K, "aiko.conv_glds_tail_decode_out: w [N, ceil64(R*R*Cc)]");
  TORCH_CHECK(w2.dim() == 2 && w2.is_contiguous() && w2.size(0) == N && w2.size(1) >= (N + 31) / 32 * 32 && w2.size(1) % 8 == 0,
              "aiko.conv_glds_tail_decode_out: w2 [N, >= ceil32(N)]");
  const int64_t Ho = H + 2 * pad - R + 1, Wo = W + 2 * pad - R + 1;
  TORCH_CHECK(boxes.scalar_type() == at::kFloat && boxes.dim() == 3 && boxes.size(0) == B && boxes.size(2) == 4 &&
                  boxes.is_contiguous() && scores.scalar_type() == at::kFloat && scores.dim() == 2 && scores.is_contiguous() &&
                  cls.scalar_type() == at::kInt && cls.dim() == 2 && cls.is_contiguous() && scores.size(0) == B &&
                  cls.size(0) == B && scores.size(1) == boxes.size(1) && cls.size(1) == boxes.size(1) &&
                  astart >= 0 && astart + Ho * Wo <= boxes.size(1),
              "aiko.conv_glds_tail_decode_out: boxes [B, A, 4] f32, scores [B, A] f32, cls [B, A] i32 covering the level");
  const int dec[5] = {(int)mode, (int)nc, (int)level_stride, (int)astart, (int)boxes.size(1)};
  check_launch(aiko_conv_glds_tail(x.data_ptr(), w.data_ptr(), bias.data_ptr<float>(), (int)H, (int)W, (int)C, (int)Cc,
                                   (int)R, (int)R, 1, (int)pad, (int)Ho, (int)Wo, (int)(B * Ho * Wo), (int)K, (int)N, (int)act,
                                   w2.data_ptr(), b2.data_ptr<float>(), nullptr, 0, (int)w2.size(1), 0, zero.data_ptr(), dec,
                                   boxes.data_ptr(), scores.data_ptr<float>(), cls.data_ptr<int>(), cur_stream()),
               "conv_glds_tail_decode");
}


// A whole ResNet stage-1 bottleneck in one launch (bneck_fused.hip): x [B, H, 56, cin] ->
// y [B, H, 56, 256]; cin 256 = identity block (w3 [256, 64]), cin 64 = projection block with
// w3 = [conv3 | shortcut] [256, 128] (K-concatenated, ops.conv.fuse_shortcut).
void bneck_fused_out(const at::Tensor& x, const at::Tensor& w1, const at::Tensor& b1, const at::Tensor& w2,
                     const at::Tensor& b2, const at::Tensor& w3, const at::Tensor& b3, at::Tensor& y, int64_t grid,
                     const c10::optional<at::Tensor>& dbg) {
  for (const at::Tensor* t : {&x, &w1, &b1, &w2, &b2, &w3, &b3, (const at::Tensor*)&y}) {
    check_cuda(*t, "bneck_fused operand");
    TORCH_CHECK(t->is_contiguous() && reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "aiko.bneck_fused_out: operands must be contiguous and 16-byte aligned");
  }
  for (const at::Tensor* t : {&x, &w1, &w2, &w3, (const at::Tensor*)&y})
    TORCH_CHECK(t->scalar_type() == at::kBFloat16, "aiko.bneck_fused_out: bf16 activations / weights");
  for (const at::Tensor* t : {&b1, &b2, &b3})
    TORCH_CHECK(t->scalar_type() == at::kFloat, "aiko.bneck_fused_out: fp32 biases");
  TORCH_CHECK(x.dim() == 4 && y.dim() == 4, "aiko.bneck_fused_out: x / y NHWC");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), cin = x.size(3);
  TORCH_CHECK(W == 56 && (cin == 256 || cin == 64), "aiko.bneck_fused_out: x must be [B, H, 56, 256 | 64]");
  TORCH_CHECK(y.size(0) == B && y.size(1) == H && y.size(2) == W && y.size(3) == 256,
              "aiko.bneck_fused_out: y must be [B, H, 56, 256]");
  const int64_t k3 = cin == 64 ? 128 : 64;
  TORCH_CHECK(w1.dim() == 2 && w1.size(0) == 64 && w1.size(1) == cin, "aiko.bneck_fused_out: w1 [64, cin]");
  TORCH_CHECK(w2.dim() == 2 && w2.size(0) == 64 && w2.size(1) == 576, "aiko.bneck_fused_out: w2 [64, 576] (3x3, tap-major)");
  TORCH_CHECK(w3.dim() == 2 && w3.size(0) == 256 && w3.size(1) == k3, "aiko.bneck_fused_out: w3 [256, ", k3, "]");
  TORCH_CHECK(b1.numel() == 64 && b2.numel() == 64 && b3.numel() == 256, "aiko.bneck_fused_out: biases [64], [64], [256]");
  TORCH_CHECK(x.data_ptr() != y.data_ptr(), "aiko.bneck_fused_out: in place is not supported");
  TORCH_CHECK(grid >= 0, "aiko.bneck_fused_out: grid must be >= 0 (0: one workgroup per CU)");
  unsigned* dbg_ptr = nullptr;
  if (dbg.has_value()) {                // diagnostics: [grid, B * H / grid + 1, 8] int32 stamps
    check_cuda(*dbg, "bneck_fused dbg");
    TORCH_CHECK(grid > 0 && dbg->scalar_type() == at::kInt && dbg->is_contiguous() &&
                    dbg->numel() >= grid * ((x.size(0) * x.size(1)) / grid + 1) * 8,
                "aiko.bneck_fused_out: dbg must be int32 [grid, B*H/grid + 1, 8] with an explicit grid");
    dbg_ptr = reinterpret_cast<unsigned*>(dbg->data_ptr());
  }
  TORCH_CHECK(B * H * W * 256 < INT_MAX, "aiko.bneck_fused_out: batch too large for 32-bit pixel indices");
  check_launch(aiko_bneck_fused(x.data_ptr(), w1.data_ptr(), b1.data_ptr<float>(), w2.data_ptr(), b2.data_ptr<float>(),
                                w3.data_ptr(), b3.data_ptr<float>(), y.data_ptr(), (int)B, (int)H, (int)W, (int)cin,
                                (int)grid, dbg_ptr, cur_stream()),
               "bneck_fused");
}

// A bottleneck's 3x3 conv + 1x1 expansion + identity residual + ReLU in one launch
// (conv_exp.hip): t1 [B, H, W, 256] -> y [B, H, W, N], N % 256 == 0; w2 [256, 2304] (3x3,
// tap-major); w3 the MFMA fragment image of the [N, 256] expansion weight
// (ops.conv.exp_weight: [N / 16, 8, 64, 8]); res [B, H, W, N].  grid: workgroups (0: one per
// 256-pixel tile).  Allocates nothing and does not synchronise.
void conv3x3_exp_out(const at::Tensor& t1, const at::Tensor& w2, const at::Tensor& b2, const at::Tensor& w3,
                     const at::Tensor& b3, const at::Tensor& res, at::Tensor& y, int64_t grid) {
  for (const at::Tensor* t : {&t1, &w2, &b2, &w3, &b3, &res, (const at::Tensor*)&y}) {
    check_cuda(*t, "conv3x3_exp operand");
    TORCH_CHECK(t->is_contiguous() && reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "aiko.conv3x3_exp_out: operands must be contiguous and 16-byte aligned");
  }
  for (const at::Tensor* t : {&t1, &w2, &w3, &res, (const at::Tensor*)&y})
    TORCH_CHECK(t->scalar_type() == at::kBFloat16, "aiko.conv3x3_exp_out: bf16 activations / weights");
  for (const at::Tensor* t : {&b2, &b3})
    TORCH_CHECK(t->scalar_type() == at::kFloat, "aiko.conv3x3_exp_out: fp32 biases");
  TORCH_CHECK(t1.dim() == 4 && t1.size(3) == 256, "aiko.conv3x3_exp_out: t1 must be [B, H, W, 256] NHWC");
  const int64_t B = t1.size(0), H = t1.size(1), W = t1.size(2);
  TORCH_CHECK(y.dim() == 4 && y.size(0) == B && y.size(1) == H && y.size(2) == W, "aiko.conv3x3_exp_out: y must be [B, H, W, N]");
  const int64_t N = y.size(3);
  TORCH_CHECK(N > 0 && N % 256 == 0, "aiko.conv3x3_exp_out: N must be a multiple of 256");
  TORCH_CHECK(res.sizes() == y.sizes(), "aiko.conv3x3_exp_out: res must have y's shape (identity residual)");
  TORCH_CHECK(w2.numel() == 256 * 9 * 256 && w2.size(0) == 256, "aiko.conv3x3_exp_out: w2 [256, 2304] (3x3, tap-major)");
  TORCH_CHECK(w3.numel() == N * 256, "aiko.conv3x3_exp_out: w3 must be the [N / 16, 8, 64, 8] fragment image");
  TORCH_CHECK(b2.numel() == 256 && b3.numel() == N, "aiko.conv3x3_exp_out: biases [256], [N]");
  TORCH_CHECK(y.data_ptr() != res.data_ptr() && y.data_ptr() != t1.data_ptr(), "aiko.conv3x3_exp_out: in place is not supported");
  TORCH_CHECK(grid >= 0, "aiko.conv3x3_exp_out: grid must be >= 0 (0: one workgroup per tile)");
  TORCH_CHECK(B > 0 && H > 0 && W > 0 && B * H * W * N * 2 < 0x7ffffff0LL,
              "aiko.conv3x3_exp_out: tensors too large for 32-bit offsets");
  check_launch(aiko_conv3x3_exp(t1.data_ptr(), w2.data_ptr(), b2.data_ptr<float>(), w3.data_ptr(), b3.data_ptr<float>(),
                                res.data_ptr(), y.data_ptr(), (int)B, (int)H, (int)W, (int)N, (int)grid, cur_stream()),
               "conv3x3_exp");
}

// uint8 frames -> letterbox/normalise -> k x k stem conv (+bias, act) -> bf16 NHWC ``out``
// [B, H1, W1, Cout]; w bf16 [Cout, 64] (k = tap * 4 + channel, zero padded); geom = [Ho, Wo, Hc, Wc, off_t, off_l, k, stride, pad, act]
void stem_direct_out(const at::Tensor& frames, const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                     at::Tensor& out, at::IntArrayRef geom, double fill, at::ArrayRef<double> mean,
                     at::ArrayRef<double> std, bool bgr) {
  check_cuda(frames, "frames");
  check_cuda(w, "w");
  check_cuda(out, "out");
  TORCH_CHECK(frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3 && frames.is_contiguous(),
              "aiko.stem_direct_out: frames must be uint8 [B, H, W, 3] contiguous");
  TORCH_CHECK(geom.size() == 10, "aiko.stem_direct_out: geom = [Ho, Wo, Hc, Wc, off_t, off_l, k, stride, pad, act]");
  const int64_t Ho = geom[0], Wo = geom[1], Hc = geom[2], Wc = geom[3], off_t = geom[4], off_l = geom[5];
  const int64_t k = geom[6], stride = geom[7], pad = geom[8], act = geom[9];
  TORCH_CHECK(off_t >= 0 && off_l >= 0 && off_t + Ho <= Hc && off_l + Wo <= Wc,
              "aiko.stem_direct_out: image must lie inside the canvas");
  const int64_t B = frames.size(0), Cout = out.size(3);
  const int64_t H1 = (Hc + 2 * pad - k) / stride + 1, W1 = (Wc + 2 * pad - k) / stride + 1;
  TORCH_CHECK(out.size(0) == B && out.size(1) == H1 && out.size(2) == W1, "aiko.stem_direct_out: out must be [B, ",
              H1, ", ", W1, ", Cout]");
  const int64_t ldo = pixel_pitch(out, "stem_direct_out");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 && w.is_contiguous() && w.dim() == 2 && w.size(0) == Cout &&
                  w.size(1) == 64 && k * k * 4 <= 64 && Cout % 16 == 0,
              "aiko.stem_direct_out: w bf16 [Cout, 64] contiguous (k <= 4, Cout % 16 == 0)");
  const float* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == Cout && bias->is_contiguous(), "aiko.stem_direct_out: bias fp32 [Cout]");
    bp = bias->data_ptr<float>();
  }
  TORCH_CHECK(mean.size() == 3 && std.size() == 3, "aiko.stem_direct_out: mean/std need 3 values");
  float m[3] = {(float)mean[0], (float)mean[1], (float)mean[2]};
  float s[3] = {(float)std[0], (float)std[1], (float)std[2]};
  check_launch(aiko_stem_direct(frames.data_ptr(), out.data_ptr(), w.data_ptr(), bp, B, frames.size(1),
                                frames.size(2), Ho, Wo, Hc, Wc, off_t, off_l, (float)fill, m, s, bgr ? 1 : 0, H1, W1,
                                Cout, ldo, k, stride, pad, act, cur_stream()),
               "stem_direct");
}

// NHWC bf16 tensor whose channels may be a slice of a wider buffer: returns the pixel pitch
int64_t pixel_pitch(const at::Tensor& t, const char* op) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.dim() == 4, "aiko.", op, ": NHWC bf16 tensors required");
  const int64_t C = t.size(3), ld = t.stride(2);
  TORCH_CHECK(t.stride(3) == 1 && t.stride(1) == t.size(2) * ld && t.stride(0) == t.size(1) * t.stride(1) &&
                  ld % 8 == 0 && C % 8 == 0 && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "aiko.", op, ": tensor must be NHWC with unit channel stride, C and pitch multiples of 8");
  TORCH_CHECK(avail_elems(t) >= (t.size(0) * t.size(1) * t.size(2) - 1) * ld + C, "aiko.", op, ": storage too small");
  return ld;
}

void maxpool_out(const at::Tensor& x, at::Tensor& y, int64_t k, int64_t s, int64_t p) {
  check_cuda(x, "x");
  check_cuda(y, "y");
  const int64_t ldx = pixel_pitch(x, "maxpool_out"), ldy = pixel_pitch(y, "maxpool_out");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  TORCH_CHECK(y.size(0) == B && y.size(3) == C, "aiko.maxpool_out: bad shapes");
  const int64_t Ho = (H + 2 * p - k) / s + 1, Wo = (W + 2 * p - k) / s + 1;
  TORCH_CHECK(y.size(1) == Ho && y.size(2) == Wo, "aiko.maxpool_out: y must be [B, ", Ho, ", ", Wo, ", C]");
  check_launch(aiko_maxpool(x.data_ptr(), y.data_ptr(), B, H, W, C, Ho, Wo, k, s, p, ldx, ldy,
                            cur_stream()),
               "maxpool");
}

// Fused 7x7/s2 stem conv + bias + ReLU + 3x3/s2/p1 max-pool (stem_pool.hip).  x: the zero-bordered
// [B, Hp, Wp, 4] preprocess buffer; w: [7, 64, 32] LDS image of the stem weights (16-byte chunks
// XOR-swizzled by channel >> 2, built by ops.conv.stem_pool); y: [B, Hm, Wm, 64] (slice ok).
void stem_pool_out(const at::Tensor& x, const at::Tensor& w, const at::Tensor& bias, at::Tensor& y,
                   int64_t Ho, int64_t Wo, int64_t variant) {
  check_cuda(x, "x");
  check_cuda(w, "w");
  check_cuda(bias, "bias");
  check_cuda(y, "y");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.dim() == 4 && x.size(3) == 4 && x.is_contiguous(),
              "aiko.stem_pool_out: x must be a contiguous [B, Hp, Wp, 4] bf16 stem buffer");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 && w.dim() == 3 && w.size(0) == 7 && w.size(1) == 64 &&
                  w.size(2) == 32 && w.is_contiguous(),
              "aiko.stem_pool_out: w must be the [7, 64, 32] swizzled stem weight image (ops.conv.stem_pool)");
  TORCH_CHECK(bias.scalar_type() == at::kFloat && bias.numel() == 64 && bias.is_contiguous(),
              "aiko.stem_pool_out: bias must be fp32 [64]");
  const int64_t ldy = pixel_pitch(y, "stem_pool_out");
  const int64_t B = x.size(0), Hp = x.size(1), Wp = x.size(2);
  const int64_t Hm = (Ho + 2 - 3) / 2 + 1, Wm = (Wo + 2 - 3) / 2 + 1;
  TORCH_CHECK(Ho > 0 && Wo > 0 && Hp >= 2 * (Ho - 1) + 7 && Wp >= 2 * (Wo - 1) + 8,
              "aiko.stem_pool_out: stem buffer too small for a ", Ho, "x", Wo, " stem output");
  TORCH_CHECK(y.size(0) == B && y.size(1) == Hm && y.size(2) == Wm && y.size(3) == 64,
              "aiko.stem_pool_out: y must be [B, ", Hm, ", ", Wm, ", 64]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(bias.data_ptr()) % 16 == 0,
              "aiko.stem_pool_out: operands must be 16-byte aligned");
  check_launch(aiko_stem_pool(x.data_ptr(), w.data_ptr(), bias.data_ptr<float>(), y.data_ptr(), B, Hp, Wp,
                              Ho, Wo, Hm, Wm, ldy, (int)variant, cur_stream()),
               "stem_pool");
}

// The same fused stem fed with uint8 frames [B, Hi, Wi, 3] (Wi % 4 == 0) — no pre-processing
// kernel, no bf16 stem buffer: w is the weight image scaled by 1 / (255 std_c)
// (ops.conv.stem_pool_u8), mean255 the per-channel 255 * mean subtracted in the kernel.
void stem_pool_u8_out(const at::Tensor& frames, const at::Tensor& w, const at::Tensor& bias, at::Tensor& y,
                      at::ArrayRef<double> mean255, int64_t variant) {
  check_cuda(frames, "frames");
  check_cuda(w, "w");
  check_cuda(bias, "bias");
  check_cuda(y, "y");
  TORCH_CHECK(frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3 && frames.is_contiguous() &&
                  frames.size(2) % 4 == 0,
              "aiko.stem_pool_u8_out: frames must be contiguous uint8 [B, H, W, 3] with W % 4 == 0");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 && w.dim() == 3 && w.size(0) == 7 && w.size(1) == 64 &&
                  w.size(2) == 32 && w.is_contiguous(),
              "aiko.stem_pool_u8_out: w must be the [7, 64, 32] swizzled stem weight image");
  TORCH_CHECK(bias.scalar_type() == at::kFloat && bias.numel() == 64 && bias.is_contiguous(),
              "aiko.stem_pool_u8_out: bias must be fp32 [64]");
  TORCH_CHECK(mean255.size() == 3, "aiko.stem_pool_u8_out: mean255 has 3 values");
  const int64_t B = frames.size(0), Hi = frames.size(1), Wi = frames.size(2);
  const int64_t Ho = (Hi + 6 - 7) / 2 + 1, Wo = (Wi + 6 - 7) / 2 + 1;
  const int64_t Hm = (Ho + 2 - 3) / 2 + 1, Wm = (Wo + 2 - 3) / 2 + 1;
  const int64_t ldy = pixel_pitch(y, "stem_pool_u8_out");
  TORCH_CHECK(y.size(0) == B && y.size(1) == Hm && y.size(2) == Wm && y.size(3) == 64,
              "aiko.stem_pool_u8_out: y must be [B, ", Hm, ", ", Wm, ", 64]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(frames.data_ptr()) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(bias.data_ptr()) % 16 == 0,
              "aiko.stem_pool_u8_out: frames 4-byte, w / bias 16-byte aligned");
  const float m[3] = {(float)mean255[0], (float)mean255[1], (float)mean255[2]};
  check_launch(aiko_stem_pool_u8(frames.data_ptr(), w.data_ptr(), bias.data_ptr<float>(), y.data_ptr(), B, Hi, Wi,
                                 Ho, Wo, Hm, Wm, ldy, m, (int)variant, cur_stream()),
               "stem_pool_u8");
}

void resize_u8_out(const at::Tensor& x, at::Tensor& y) {
  check_cuda(x, "x");
  check_cuda(y, "y");
  TORCH_CHECK(x.scalar_type() == at::kByte && y.scalar_type() == at::kByte && x.dim() == 4 && y.dim() == 4 &&
                  x.size(3) == 3 && y.size(3) == 3 && x.is_contiguous() && y.is_contiguous() && x.size(0) == y.size(0),
              "aiko.resize_u8_out: uint8 [B, H, W, 3] contiguous tensors required");
  check_launch(aiko_resize_u8(x.data_ptr(), y.data_ptr(), x.size(0), x.size(1), x.size(2), y.size(1), y.size(2),
                              cur_stream()),
               "resize_u8");
}

// crops[b*k + i] <- the rect of det[b, i] (i < min(count[b], k), coordinates finite) resized to
// crops' [Ho, Wo]; rois[b*k + i] <- that rect (x0, y0, x1, y1), half-open; other slots zero
void roi_crop_out(const at::Tensor& frames, const at::Tensor& det, const at::Tensor& count, int64_t k,
                  double margin, at::Tensor& crops, at::Tensor& rois) {
  check_cuda(frames, "frames");
  check_cuda(det, "det");
  check_cuda(count, "count");
  check_cuda(crops, "crops");
  check_cuda(rois, "rois");
  TORCH_CHECK(frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3 &&
                  frames.is_contiguous() && frames.numel() >= 4,
              "aiko.roi_crop_out: frames uint8 [B, H, W, 3] contiguous required");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  TORCH_CHECK(det.scalar_type() == at::kFloat && det.dim() == 3 && det.size(0) == B && det.size(2) == 6 &&
                  det.is_contiguous(),
              "aiko.roi_crop_out: det fp32 [B, max_det, 6] contiguous required");
  TORCH_CHECK(count.scalar_type() == at::kInt && count.dim() == 1 && count.size(0) == B && count.is_contiguous(),
              "aiko.roi_crop_out: count int32 [B] required");
  const int64_t max_det = det.size(1);
  TORCH_CHECK(k >= 1 && k <= max_det, "aiko.roi_crop_out: 1 <= k <= max_det (", max_det, ") required, got ", k);
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
  TORCH_CHECK(reinterpret_cast<uintptr_t>(crops.data_ptr()) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(rois.data_ptr()) % 16 == 0,
              "aiko.roi_crop_out: crops 4-byte, rois 16-byte aligned");
  check_launch(aiko_roi_crop_u8(frames.data_ptr(), det.data_ptr<float>(), count.data_ptr<int>(), crops.data_ptr(),
                                rois.data_ptr<int>(), B, H, W, max_det, k, Ho, Wo, (float)margin, cur_stream()),
               "roi_crop_u8");
}

// out <- frames with the boxes and labels of det[b, i] (i < min(count[b], k), coordinates finite)
// drawn over them; slot b*k + i of labels / scores overrides the detector's class / score.  out may
// be frames itself (drawn in place)
void draw_detections_out(const at::Tensor& frames, const at::Tensor& det, const at::Tensor& count, int64_t k,
                         const c10::optional<at::Tensor>& labels, const c10::optional<at::Tensor>& scores,
                         const at::Tensor& names, const at::Tensor& font, const at::Tensor& palette,
                         int64_t glyph_width, int64_t thickness, int64_t text_scale, double margin, bool show_score,
                         at::Tensor& out) {
  check_cuda(frames, "frames");
  check_cuda(det, "det");
  check_cuda(count, "count");
  check_cuda(names, "names");
  check_cuda(font, "font");
  check_cuda(palette, "palette");
  check_cuda(out, "out");
  TORCH_CHECK(frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3 &&
                  frames.is_contiguous() && frames.numel() >= 3,
              "aiko.draw_detections_out: frames uint8 [B, H, W, 3] contiguous required");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  TORCH_CHECK(det.scalar_type() == at::kFloat && det.dim() == 3 && det.size(0) == B && det.size(2) == 6 &&
                  det.is_contiguous(),
              "aiko.draw_detections_out: det fp32 [B, max_det, 6] contiguous required");
  TORCH_CHECK(count.scalar_type() == at::kInt && count.dim() == 1 && count.size(0) == B && count.is_contiguous(),
              "aiko.draw_detections_out: count int32 [B] required");
  const int64_t max_det = det.size(1);
  TORCH_CHECK(k >= 1 && k <= max_det, "aiko.draw_detections_out: 1 <= k <= max_det (", max_det, ") required, got ", k);
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
  const auto fp = reinterpret_cast<uintptr_t>(frames.data_ptr()), op = reinterpret_cast<uintptr_t>(out.data_ptr());
  const uintptr_t nbytes = (uintptr_t)frames.numel();
  TORCH_CHECK(fp == op || fp + nbytes <= op || op + nbytes <= fp,
              "aiko.draw_detections_out: out overlaps frames without being the same tensor");
  TORCH_CHECK(B <= 65535 && (H + 31) / 32 <= 65535 && H <= (1 << 24) && W <= (1 << 24),
              "aiko.draw_detections_out: B = ", B, ", H = ", H, ", W = ", W,
              " exceed the grid limit (65535 frames, 65535 tile rows of 32, side <= 2^24)");
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
  check_cuda(frames, "frames");
  check_cuda(det, "det");
  check_cuda(count, "count");
  check_cuda(out, "out");
  TORCH_CHECK(frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3 &&
                  frames.is_contiguous() && frames.numel() >= 3,
              "aiko.redact_detections_out: frames uint8 [B, H, W, 3] contiguous required");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  TORCH_CHECK(det.scalar_type() == at::kFloat && det.dim() == 3 && det.size(0) == B && det.size(2) == 6 &&
                  det.is_contiguous(),
              "aiko.redact_detections_out: det fp32 [B, max_det, 6] contiguous required");
  TORCH_CHECK(count.scalar_type() == at::kInt && count.dim() == 1 && count.size(0) == B && count.is_contiguous(),
              "aiko.redact_detections_out: count int32 [B] required");
  const int64_t max_det = det.size(1);
  TORCH_CHECK(k >= 1 && k <= max_det, "aiko.redact_detections_out: 1 <= k <= max_det (", max_det, ") required, got ",
              k);
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
  const auto fp = reinterpret_cast<uintptr_t>(frames.data_ptr()), op = reinterpret_cast<uintptr_t>(out.data_ptr());
  const uintptr_t nbytes = (uintptr_t)frames.numel();
  TORCH_CHECK(fp == op || fp + nbytes <= op || op + nbytes <= fp,
              "aiko.redact_detections_out: out overlaps frames without being the same tensor");
  TORCH_CHECK(B <= 65535 && (H + 31) / 32 <= 65535 && H <= (1 << 24) && W <= (1 << 24),
              "aiko.redact_detections_out: B = ", B, ", H = ", H, ", W = ", W,
              " exceed the grid limit (65535 frames, 65535 tile rows of 32, side <= 2^24)");
  check_launch(aiko_redact_detections(frames.data_ptr(), out.data_ptr(), det.data_ptr<float>(), count.data_ptr<int>(),
                                      lp, sp, B, H, W, max_det, k, C, mode, block, fill_rgb, (float)margin,
                                      cur_stream()),
               "redact_detections");
}

// out [B, H, W, 3] <- raw [B, frame_bytes] YUV frames, tightly packed.  format: 0 nv12, 1 i420,
// 2 i444, 3 yuyv; coeffs: yoff, ygain, rv, gu, gv, bu; round_mode: 0 rint, 1 add half and truncate
void yuv_to_rgb_out(const at::Tensor& raw, int64_t height, int64_t width, int64_t format,
                    at::ArrayRef<double> coeffs, int64_t round_mode, at::Tensor& out) {
  check_cuda(raw, "raw");
  check_cuda(out, "out");
  TORCH_CHECK(raw.device() == out.device(), "aiko.yuv_to_rgb_out: raw and out on different devices");
  TORCH_CHECK(format >= 0 && format <= 3, "aiko.yuv_to_rgb_out: unknown format code ", format);
  TORCH_CHECK(round_mode == 0 || round_mode == 1, "aiko.yuv_to_rgb_out: unknown round mode ", round_mode);
  TORCH_CHECK(coeffs.size() == 6, "aiko.yuv_to_rgb_out: 6 coefficients (yoff, ygain, rv, gu, gv, bu) required, got ",
              coeffs.size());
  float coef[6];
  for (int i = 0; i < 6; ++i) {
    coef[i] = (float)coeffs[i];
    TORCH_CHECK(std::isfinite(coef[i]), "aiko.yuv_to_rgb_out: coefficient ", i, " is not finite in fp32");
  }
  TORCH_CHECK(height >= 1 && width >= 1 && height <= 32768 && width <= 32768,
              "aiko.yuv_to_rgb_out: 1 <= height, width <= 32768 required, got ", height, " x ", width);
  TORCH_CHECK(format != 3 || width % 2 == 0, "aiko.yuv_to_rgb_out: yuyv needs an even width, got ", width);
  const int64_t H = height, W = width, cplane = ((H + 1) / 2) * ((W + 1) / 2);
  const int64_t frame_bytes = format == 2 ? 3 * H * W : format == 3 ? 2 * H * W : H * W + 2 * cplane;
  TORCH_CHECK(raw.scalar_type() == at::kByte && raw.dim() == 2 && raw.is_contiguous() && raw.size(0) >= 1,
              "aiko.yuv_to_rgb_out: raw uint8 [B, frame_bytes] contiguous required");
  TORCH_CHECK(raw.size(1) == frame_bytes, "aiko.yuv_to_rgb_out: a ", H, " x ", W, " frame of this format has ",
              frame_bytes, " bytes, raw has ", raw.size(1));
  const int64_t B = raw.size(0);
  TORCH_CHECK(out.scalar_type() == at::kByte && out.dim() == 4 && out.size(0) == B && out.size(1) == H &&
                  out.size(2) == W && out.size(3) == 3 && out.is_contiguous(),
              "aiko.yuv_to_rgb_out: out uint8 [B, H, W, 3] contiguous required");
  TORCH_CHECK(B <= 65535, "aiko.yuv_to_rgb_out: B = ", B, " exceeds the grid limit (65535 frames)");
  const auto rp = reinterpret_cast<uintptr_t>(raw.data_ptr()), op = reinterpret_cast<uintptr_t>(out.data_ptr());
  TORCH_CHECK(rp + (uintptr_t)raw.numel() <= op || op + (uintptr_t)out.numel() <= rp,
              "aiko.yuv_to_rgb_out: raw and out overlap");
  check_launch(aiko_yuv_to_rgb_u8(raw.data_ptr(), out.data_ptr(), B, H, W, (int)format, coef, (int)round_mode,
                                  cur_stream()),
               "yuv_to_rgb_u8");
}

// out [B, frame_bytes] YUV frames, tightly packed <- rgb [B, H, W, 3].  format: 0 nv12, 1 i420,
// 2 i444, 3 yuyv; coeffs: yoff, yr, yg, yb, ur, ug, ub, vr, vg, vb; round_mode: 0 rint, 1 add half
// and truncate
void rgb_to_yuv_out(const at::Tensor& rgb, int64_t format, at::ArrayRef<double> coeffs, int64_t round_mode,
                    at::Tensor& out) {
  check_cuda(rgb, "rgb");
  check_cuda(out, "out");
  TORCH_CHECK(rgb.device() == out.device(), "aiko.rgb_to_yuv_out: rgb and out on different devices");
  TORCH_CHECK(format >= 0 && format <= 3, "aiko.rgb_to_yuv_out: unknown format code ", format);
  TORCH_CHECK(round_mode == 0 || round_mode == 1, "aiko.rgb_to_yuv_out: unknown round mode ", round_mode);
  TORCH_CHECK(coeffs.size() == 10,
              "aiko.rgb_to_yuv_out: 10 coefficients (yoff, yr, yg, yb, ur, ug, ub, vr, vg, vb) required, got ",
              coeffs.size());
  float coef[10];
  for (int i = 0; i < 10; ++i) {
    coef[i] = (float)coeffs[i];
    TORCH_CHECK(std::isfinite(coef[i]), "aiko.rgb_to_yuv_out: coefficient ", i, " is not finite in fp32");
  }
  TORCH_CHECK(rgb.scalar_type() == at::kByte && rgb.dim() == 4 && rgb.size(3) == 3 && rgb.is_contiguous() &&
                  rgb.size(0) >= 1,
              "aiko.rgb_to_yuv_out: rgb uint8 [B, H, W, 3] contiguous required");
  const int64_t B = rgb.size(0), H = rgb.size(1), W = rgb.size(2);
  TORCH_CHECK(H >= 1 && W >= 1 && H <= 32768 && W <= 32768,
              "aiko.rgb_to_yuv_out: 1 <= height, width <= 32768 required, got ", H, " x ", W);
  TORCH_CHECK(format != 3 || W % 2 == 0, "aiko.rgb_to_yuv_out: yuyv needs an even width, got ", W);
  const int64_t cplane = ((H + 1) / 2) * ((W + 1) / 2);
  const int64_t frame_bytes = format == 2 ? 3 * H * W : format == 3 ? 2 * H * W : H * W + 2 * cplane;
  TORCH_CHECK(out.scalar_type() == at::kByte && out.dim() == 2 && out.size(0) == B && out.is_contiguous(),
              "aiko.rgb_to_yuv_out: out uint8 [B, frame_bytes] contiguous required");
  TORCH_CHECK(out.size(1) == frame_bytes, "aiko.rgb_to_yuv_out: a ", H, " x ", W, " frame of this format has ",
              frame_bytes, " bytes, out has ", out.size(1));
  TORCH_CHECK(B <= 65535, "aiko.rgb_to_yuv_out: B = ", B, " exceeds the grid limit (65535 frames)");
  const auto rp = reinterpret_cast<uintptr_t>(rgb.data_ptr()), op = reinterpret_cast<uintptr_t>(out.data_ptr());
  TORCH_CHECK(rp + (uintptr_t)rgb.numel() <= op || op + (uintptr_t)out.numel() <= rp,
              "aiko.rgb_to_yuv_out: rgb and out overlap");
  check_launch(aiko_rgb_to_yuv_u8(rgb.data_ptr(), out.data_ptr(), B, H, W, (int)format, coef, (int)round_mode,
                                  cur_stream()),
               "rgb_to_yuv_u8");
}

void batchnorm_out(const at::Tensor& x, const at::Tensor& scale, const at::Tensor& shift, at::Tensor& y, int64_t act) {
  check_cuda(x, "x");
  check_cuda(y, "y");
  check_cuda(scale, "scale");
  check_cuda(shift, "shift");
  const int64_t ldx = pixel_pitch(x, "batchnorm_out"), ldy = pixel_pitch(y, "batchnorm_out");
  const int64_t C = x.size(3);
  TORCH_CHECK(y.sizes() == x.sizes(), "aiko.batchnorm_out: y must match x");
  TORCH_CHECK(scale.scalar_type() == at::kFloat && shift.scalar_type() == at::kFloat && scale.numel() == C &&
                  shift.numel() == C && scale.is_contiguous() && shift.is_contiguous(),
              "aiko.batchnorm_out: scale/shift fp32 [C]");
  check_launch(aiko_batchnorm(x.data_ptr(), y.data_ptr(), scale.data_ptr<float>(), shift.data_ptr<float>(),
                              x.size(0) * x.size(1) * x.size(2), C, ldx, ldy, act, cur_stream()),
               "batchnorm");
}

void upsample2x_out(const at::Tensor& x, at::Tensor& y) {
  check_cuda(x, "x");
  check_cuda(y, "y");
  const int64_t ldx = pixel_pitch(x, "upsample2x_out"), ldy = pixel_pitch(y, "upsample2x_out");
  TORCH_CHECK(y.size(0) == x.size(0) && y.size(1) == 2 * x.size(1) && y.size(2) == 2 * x.size(2) &&
                  y.size(3) == x.size(3),
              "aiko.upsample2x_out: y must be [B, 2H, 2W, C]");
  check_launch(aiko_upsample2x(x.data_ptr(), y.data_ptr(), x.size(0), x.size(1), x.size(2), x.size(3),
                               ldx, ldy, cur_stream()),
               "upsample2x");
}

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
  check_cuda(boxes, "boxes");
  check_cuda(scores, "scores");
  check_cuda(cls, "cls");
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
  check_cuda(boxes, "boxes");
  check_cuda(scores, "scores");
  check_cuda(cls, "cls");
  check_cuda(det, "det");
  check_cuda(count, "count");
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
  TORCH_CHECK(det.scalar_type() == at::kFloat && det.dim() == 3 && det.size(0) == B && det.size(2) == 6 &&
                  det.is_contiguous(),
              "aiko.topk_nms_out: det fp32 [B, max_det, 6]");
  const int64_t max_det = det.size(1);
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

void mean_rows_out(const at::Tensor& x, at::Tensor& y) {
  check_cuda(x, "x");
  check_cuda(y, "y");
  // x may be a T-prefix view of a [B, Tp, C] buffer: rows contiguous, any batch pitch >= T*C
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.dim() == 3 && x.stride(2) == 1 &&
                  x.stride(1) == x.size(2) && x.stride(0) >= x.size(1) * x.size(2) &&
                  y.scalar_type() == at::kFloat && y.is_contiguous(),
              "aiko.mean_rows_out: x bf16 [B, T, C] with contiguous rows, y fp32 [B, C]");
  const int64_t B = x.size(0), T = x.size(1), C = x.size(2);
  TORCH_CHECK(C % 8 == 0 && y.numel() == B * C, "aiko.mean_rows_out: C % 8 == 0, y [B, C]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && x.stride(0) % 8 == 0,
              "aiko.mean_rows_out: 16-byte aligned rows");
  TORCH_CHECK(avail_elems(x) >= (B - 1) * x.stride(0) + T * C, "aiko.mean_rows_out: x storage too small");
  check_launch(aiko_mean_rows_f32(x.data_ptr(), y.data_ptr<float>(), B, T, C, (long)x.stride(0), cur_stream()),
               "mean_rows");
}

// SPPF: slices 1..3 of the [B, H, W, >= 4c] concat buffer = chained k x k / 1 max pools of slice 0
void sppf_pool_(at::Tensor& cat, int64_t c, int64_t k) {
  check_cuda(cat, "cat");
  const int64_t ld = pixel_pitch(cat, "sppf_pool_");
  TORCH_CHECK(c % 8 == 0 && 4 * c <= cat.size(3) && k % 2 == 1 && cat.size(1) * cat.size(2) <= 2048,
              "aiko.sppf_pool_: c % 8 == 0, 4c <= C, odd k, H*W <= 2048");
  check_launch(aiko_sppf_pool(cat.data_ptr(), cat.size(0), cat.size(1), cat.size(2), (int)ld, (int)c, (int)k,
                              cur_stream()), "sppf_pool");
}

void zero_border_rows_(at::Tensor& x, int64_t rows) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.is_contiguous() && x.size(1) % 8 == 0 &&
                  rows >= 2 && x.size(0) % rows == 0,
              "aiko.zero_border_rows_: x bf16 [B*rows, C] contiguous, C % 8 == 0");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "aiko.zero_border_rows_: alignment");
  check_launch(aiko_zero_border_rows(x.data_ptr(), x.size(0) / rows, rows, x.size(1), cur_stream()),
               "zero_border_rows");
}

void window_shift_out(const at::Tensor& src, const at::Tensor& chunk, at::Tensor& dst) {
  check_cuda(src, "src");
  check_cuda(chunk, "chunk");
  check_cuda(dst, "dst");
  TORCH_CHECK(src.scalar_type() == at::kFloat && chunk.scalar_type() == at::kFloat && dst.scalar_type() == at::kFloat &&
                  src.dim() == 2 && chunk.dim() == 2 && src.sizes() == dst.sizes() && src.is_contiguous() &&
                  chunk.is_contiguous() && dst.is_contiguous() && chunk.size(0) == src.size(0),
              "aiko.window_shift_out: fp32 contiguous src / dst [B, W], chunk [B, n]");
  TORCH_CHECK(src.data_ptr() != dst.data_ptr(), "aiko.window_shift_out: dst must not alias src");
  const int64_t B = src.size(0), W = src.size(1), n = chunk.size(1);
  TORCH_CHECK(n <= W && W % 4 == 0 && n % 4 == 0, "aiko.window_shift_out: n <= W, both multiples of 4");
  check_launch(aiko_window_shift(src.data_ptr<float>(), chunk.data_ptr<float>(), dst.data_ptr<float>(), B, W, n,
                                 cur_stream()), "window_shift");
}

// out [B, n_in L / M], hist_out [B, T-1] <- pcm [B, n_in, C] (int16 or fp32, interleaved), the
// stream's previous T-1 mono samples hist [B, T-1] and the polyphase taps filt [L, T]
// (resample_ops.hip; the arithmetic is in ops/audio.py)
void resample_out(const at::Tensor& pcm, const at::Tensor& hist, const at::Tensor& filt, int64_t L, int64_t M,
                  at::Tensor& out, at::Tensor& hist_out) {
  check_cuda(pcm, "pcm");
  check_cuda(hist, "hist");
  check_cuda(filt, "filt");
  check_cuda(out, "out");
  check_cuda(hist_out, "hist_out");
  TORCH_CHECK(pcm.device() == hist.device() && pcm.device() == filt.device() && pcm.device() == out.device() &&
                  pcm.device() == hist_out.device(),
              "aiko.resample_out: tensors on different devices");
  TORCH_CHECK((pcm.scalar_type() == at::kShort || pcm.scalar_type() == at::kFloat) && pcm.dim() == 3 &&
                  pcm.is_contiguous() && pcm.size(0) >= 1 && pcm.size(1) >= 1,
              "aiko.resample_out: pcm int16 or fp32 [B, n_in, C] contiguous required");
  const int64_t B = pcm.size(0), n_in = pcm.size(1), C = pcm.size(2);
  TORCH_CHECK(C >= 1 && C <= 8, "aiko.resample_out: 1 <= C <= 8 channels required, got ", C);
  TORCH_CHECK(L >= 1 && M >= 1 && L <= 16384 && M <= (1 << 24), "aiko.resample_out: bad ratio L / M = ", L, " / ", M);
  TORCH_CHECK(filt.scalar_type() == at::kFloat && filt.dim() == 2 && filt.size(0) == L && filt.size(1) >= 1 &&
                  filt.is_contiguous(),
              "aiko.resample_out: filt fp32 [L, T] contiguous required, L = ", L);
  const int64_t T = filt.size(1);
  TORCH_CHECK(L * T <= 16384, "aiko.resample_out: L * T = ", L * T, " taps exceed 16384 (64 KiB)");
  const int64_t span = (1023 * M + L - 1) / L + T;     // samples a tile of 1024 outputs reads
  TORCH_CHECK(4 * (L * T + span) <= 160 * 1024, "aiko.resample_out: taps and a tile's ", span,
              " samples exceed 160 KiB of LDS (M / L too large)");
  TORCH_CHECK(n_in <= (1 << 30) && n_in * C <= (1 << 30), "aiko.resample_out: n_in * C = ", n_in * C,
              " exceeds 2^30");
  TORCH_CHECK(n_in * L % M == 0, "aiko.resample_out: n_in * L % M != 0 (n_in = ", n_in, ", L / M = ", L, " / ", M,
              "): a chunk must end at phase 0");
  const int64_t n_out = n_in * L / M;
  TORCH_CHECK(n_out <= (1 << 30), "aiko.resample_out: n_out = ", n_out, " exceeds 2^30");
  TORCH_CHECK(hist.scalar_type() == at::kFloat && hist.dim() == 2 && hist.size(0) == B && hist.size(1) == T - 1 &&
                  hist.is_contiguous(),
              "aiko.resample_out: hist fp32 [B, T-1] = [", B, ", ", T - 1, "] contiguous required");
  TORCH_CHECK(hist_out.scalar_type() == at::kFloat && hist_out.dim() == 2 && hist_out.size(0) == B &&
                  hist_out.size(1) == T - 1 && hist_out.is_contiguous(),
              "aiko.resample_out: hist_out fp32 [B, T-1] = [", B, ", ", T - 1, "] contiguous required");
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.dim() == 2 && out.size(0) == B && out.size(1) == n_out &&
                  out.is_contiguous(),
              "aiko.resample_out: out fp32 [B, n_out] = [", B, ", ", n_out, "] contiguous required");
  TORCH_CHECK(B <= 65535, "aiko.resample_out: B = ", B, " exceeds the grid limit (65535 streams)");
  // neither output may overlap an input or the other output
  const at::Tensor* ins[3] = {&pcm, &hist, &filt};
  const char* in_names[3] = {"pcm", "hist", "filt"};
  const at::Tensor* outs[2] = {&out, &hist_out};
  const char* out_names[2] = {"out", "hist_out"};
  auto overlap = [](const at::Tensor& x, const at::Tensor& y) {
    const auto xp = reinterpret_cast<uintptr_t>(x.data_ptr()), yp = reinterpret_cast<uintptr_t>(y.data_ptr());
    const uintptr_t xn = x.numel() * x.element_size(), yn = y.numel() * y.element_size();
    return xn > 0 && yn > 0 && xp < yp + yn && yp < xp + xn;
  };
  for (int o = 0; o < 2; ++o) {
    for (int i = 0; i < 3; ++i)
      TORCH_CHECK(!overlap(*outs[o], *ins[i]), "aiko.resample_out: ", out_names[o], " and ", in_names[i], " overlap");
  }
  TORCH_CHECK(!overlap(out, hist_out), "aiko.resample_out: out and hist_out overlap");
  check_launch(aiko_resample(pcm.data_ptr(), pcm.scalar_type() == at::kFloat ? 1 : 0, hist.data_ptr<float>(),
                             filt.data_ptr<float>(), out.data_ptr<float>(), hist_out.data_ptr<float>(), (int)B,
                             (long)n_in, (int)C, (int)L, (int)M, (int)T, cur_stream()),
               "resample");
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
  for (int i = 0; i < 5; ++i) check_cuda(*ins[i], in_names[i]);
  for (int o = 0; o < 6; ++o) check_cuda(*outs[o], out_names[o]);
  for (int i = 1; i < 5; ++i)
    TORCH_CHECK(ins[i]->device() == det.device(), "aiko.track_detections_out: tensors on different devices");
  for (int o = 0; o < 6; ++o)
    TORCH_CHECK(outs[o]->device() == det.device(), "aiko.track_detections_out: tensors on different devices");
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
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "aiko.track_detections_out: boxes and meta 16-byte aligned");
  // no output may overlap an input or another output
  auto overlap = [](const at::Tensor& x, const at::Tensor& y) {
    const auto xp = reinterpret_cast<uintptr_t>(x.data_ptr()), yp = reinterpret_cast<uintptr_t>(y.data_ptr());
    const uintptr_t xn = x.numel() * x.element_size(), yn = y.numel() * y.element_size();
    return xn > 0 && yn > 0 && xp < yp + yn && yp < xp + xn;
  };
  for (int o = 0; o < 6; ++o) {
    for (int i = 0; i < 5; ++i)
      TORCH_CHECK(!overlap(*outs[o], *ins[i]), "aiko.track_detections_out: ", out_names[o], " and ", in_names[i],
                  " overlap");
    for (int p = 0; p < o; ++p)
      TORCH_CHECK(!overlap(*outs[o], *outs[p]), "aiko.track_detections_out: ", out_names[o], " and ", out_names[p],
                  " overlap");
  }
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
  for (int i = 0; i < 3; ++i) check_cuda(*ins[i], in_names[i]);
  for (int o = 0; o < 6; ++o) check_cuda(*outs[o], out_names[o]);
  for (int i = 1; i < 3; ++i)
    TORCH_CHECK(ins[i]->device() == frames.device(), "aiko.motion_detect_out: tensors on different devices");
  for (int o = 0; o < 6; ++o)
    TORCH_CHECK(outs[o]->device() == frames.device(), "aiko.motion_detect_out: tensors on different devices");
  TORCH_CHECK(frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3 &&
                  frames.is_contiguous() && frames.numel() >= 3,
              "aiko.motion_detect_out: frames uint8 [B, H, W, 3] contiguous required");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  TORCH_CHECK(cell == 8 || cell == 16 || cell == 32, "aiko.motion_detect_out: cell in {8, 16, 32} required, got ",
              cell);
  TORCH_CHECK(B <= 65535 && (H + 31) / 32 <= 65535 && H <= (1 << 24) && W <= (1 << 24),
              "aiko.motion_detect_out: B = ", B, ", H = ", H, ", W = ", W,
              " exceed the grid limit (65535 frames, 65535 tile rows of 32, side <= 2^24)");
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
  TORCH_CHECK(det.scalar_type() == at::kFloat && det.dim() == 3 && det.size(0) == B && det.size(2) == 6 &&
                  det.is_contiguous(),
              "aiko.motion_detect_out: det fp32 [B, max_det, 6] contiguous required");
  const int64_t max_det = det.size(1);
  TORCH_CHECK(max_det >= 1 && max_det <= 64, "aiko.motion_detect_out: 1 <= max_det <= 64 required, got ", max_det);
  for (const at::Tensor* t : {&count, &cells})
    TORCH_CHECK(t->scalar_type() == at::kInt && t->dim() == 1 && t->size(0) == B && t->is_contiguous(),
                "aiko.motion_detect_out: count and cells int32 [B] contiguous required");
  TORCH_CHECK(mask.scalar_type() == at::kByte && mask.dim() == 3 && mask.size(0) == B && mask.size(1) == Gh &&
                  mask.size(2) == Gw && mask.is_contiguous(),
              "aiko.motion_detect_out: mask uint8 [B, Gh, Gw] = [", B, ", ", Gh, ", ", Gw, "] contiguous required");
  // no output may overlap an input or another output
  auto overlap = [](const at::Tensor& x, const at::Tensor& y) {
    const auto xp = reinterpret_cast<uintptr_t>(x.data_ptr()), yp = reinterpret_cast<uintptr_t>(y.data_ptr());
    const uintptr_t xn = x.numel() * x.element_size(), yn = y.numel() * y.element_size();
    return xn > 0 && yn > 0 && xp < yp + yn && yp < xp + xn;
  };
  for (int o = 0; o < 6; ++o) {
    for (int i = 0; i < 3; ++i)
      TORCH_CHECK(!overlap(*outs[o], *ins[i]), "aiko.motion_detect_out: ", out_names[o], " and ", in_names[i],
                  " overlap");
    for (int p = 0; p < o; ++p)
      TORCH_CHECK(!overlap(*outs[o], *outs[p]), "aiko.motion_detect_out: ", out_names[o], " and ", out_names[p],
                  " overlap");
  }
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
    TORCH_CHECK(outs[o]->device() == frames.device(), "aiko.marker_detect_out: tensors on different devices");
  }
  TORCH_CHECK(frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3 &&
                  frames.is_contiguous() && frames.numel() >= 3,
              "aiko.marker_detect_out: frames uint8 [B, H, W, 3] contiguous required");
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
  TORCH_CHECK(det.scalar_type() == at::kFloat && det.dim() == 3 && det.size(0) == B && det.size(2) == 6 &&
                  det.is_contiguous(),
              "aiko.marker_detect_out: det fp32 [B, max_det, 6] contiguous required");
  const int64_t max_det = det.size(1);
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
  auto overlap = [](const at::Tensor& x, const at::Tensor& y) {
    const auto xp = reinterpret_cast<uintptr_t>(x.data_ptr()), yp = reinterpret_cast<uintptr_t>(y.data_ptr());
    const uintptr_t xn = x.numel() * x.element_size(), yn = y.numel() * y.element_size();
    return xn > 0 && yn > 0 && xp < yp + yn && yp < xp + xn;
  };
  for (int o = 0; o < 7; ++o) {
    TORCH_CHECK(!overlap(*outs[o], frames), "aiko.marker_detect_out: ", out_names[o], " and frames overlap");
    for (int p = 0; p < o; ++p)
      TORCH_CHECK(!overlap(*outs[o], *outs[p]), "aiko.marker_detect_out: ", out_names[o], " and ", out_names[p],
                  " overlap");
  }
  check_launch(aiko_marker_detect(frames.data_ptr(), det.data_ptr<float>(), count.data_ptr<int>(),
                                  corners.data_ptr<int>(), ids.data_ptr<int>(), cands.data_ptr<int>(), mask.data_ptr(),
                                  work.data_ptr(), (int)B, (int)H, (int)W, (int)modules, (int)cell, (int)contrast,
                                  (int)min_side, (int)max_cand, (int)max_det, (int)passes, cur_stream()),
               "marker_detect");
}

// One voice-activity step (vad_ops.hip; the rule is in ops/vad.py): audio fp32 [B, n] at 16 kHz and the
// state [B, 8] -> the next state in state_out, per frame of ``frame`` samples level / zc / mask [B, F],
// the runs of the mask in seg [B, max_seg, 2] / count [B], the speech frames in speech [B] and
// silent [B].  Two launches on the current stream
void voice_activity_out(const at::Tensor& audio, const at::Tensor& state, int64_t frame, int64_t threshold,
                        int64_t min_level, int64_t up_shift, int64_t speech_shift, int64_t down_shift, int64_t warmup,
                        int64_t attack, int64_t hang, int64_t max_zc, int64_t window, at::Tensor& state_out,
                        at::Tensor& level, at::Tensor& zc, at::Tensor& mask, at::Tensor& seg, at::Tensor& count,
                        at::Tensor& speech, at::Tensor& silent) {
  const at::Tensor* ins[2] = {&audio, &state};
  const char* in_names[2] = {"audio", "state"};
  const at::Tensor* outs[8] = {&state_out, &level, &zc, &mask, &seg, &count, &speech, &silent};
  const char* out_names[8] = {"state_out", "level", "zc", "mask", "seg", "count", "speech", "silent"};
  for (int i = 0; i < 2; ++i) check_cuda(*ins[i], in_names[i]);
  for (int o = 0; o < 8; ++o) check_cuda(*outs[o], out_names[o]);
  TORCH_CHECK(state.device() == audio.device(), "aiko.voice_activity_out: tensors on different devices");
  for (int o = 0; o < 8; ++o)
    TORCH_CHECK(outs[o]->device() == audio.device(), "aiko.voice_activity_out: tensors on different devices");
  TORCH_CHECK(audio.scalar_type() == at::kFloat && audio.dim() == 2 && audio.is_contiguous() && audio.size(0) >= 1,
              "aiko.voice_activity_out: audio fp32 [B, n] contiguous required");
  TORCH_CHECK(frame == 160 || frame == 320 || frame == 480,
              "aiko.voice_activity_out: frame in {160, 320, 480} required, got ", frame);
  const int64_t B = audio.size(0), n = audio.size(1);
  TORCH_CHECK(n >= frame && n % frame == 0, "aiko.voice_activity_out: n % frame != 0 or n = 0 (n = ", n,
              ", frame = ", frame, "): a chunk is whole frames");
  const int64_t F = n / frame;
  TORCH_CHECK(F <= 4096, "aiko.voice_activity_out: F = ", F, " frames exceed 4096 per call");
  TORCH_CHECK(B <= 65535, "aiko.voice_activity_out: B = ", B, " exceeds the grid limit (65535 streams)");
  const struct { const char* name; int64_t v, lo, hi; } ranges[] = {
      {"threshold", threshold, 0, 1023}, {"min_level", min_level, 0, 1023}, {"up_shift", up_shift, 0, 16},
      {"speech_shift", speech_shift, 0, 16}, {"down_shift", down_shift, 0, 16}, {"warmup", warmup, 1, INT_MAX},
      {"attack", attack, 1, INT_MAX}, {"hang", hang, 0, INT_MAX}, {"max_zc", max_zc, 0, 479},
      {"window", window, 1, INT_MAX}};
  for (const auto& r : ranges)
    TORCH_CHECK(r.v >= r.lo && r.v <= r.hi, "aiko.voice_activity_out: ", r.lo, " <= ", r.name, " <= ", r.hi,
                " required, got ", r.v);
  auto is_state = [&](const at::Tensor& s) {
    return s.scalar_type() == at::kInt && s.dim() == 2 && s.size(0) == B && s.size(1) == 8 && s.is_contiguous();
  };
  TORCH_CHECK(is_state(state), "aiko.voice_activity_out: state int32 [B, 8] contiguous required, B = ", B);
  TORCH_CHECK(is_state(state_out), "aiko.voice_activity_out: state_out int32 [B, 8] contiguous required, B = ", B);
  for (const at::Tensor* t : {&level, &zc})
    TORCH_CHECK(t->scalar_type() == at::kInt && t->dim() == 2 && t->size(0) == B && t->size(1) == F &&
                    t->is_contiguous(),
                "aiko.voice_activity_out: level and zc int32 [B, F] = [", B, ", ", F, "] contiguous required");
  TORCH_CHECK(mask.scalar_type() == at::kByte && mask.dim() == 2 && mask.size(0) == B && mask.size(1) == F &&
                  mask.is_contiguous(),
              "aiko.voice_activity_out: mask uint8 [B, F] = [", B, ", ", F, "] contiguous required");
  TORCH_CHECK(seg.scalar_type() == at::kInt && seg.dim() == 3 && seg.size(0) == B && seg.size(2) == 2 &&
                  seg.is_contiguous(),
              "aiko.voice_activity_out: seg int32 [B, max_seg, 2] contiguous required");
  const int64_t max_seg = seg.size(1);
  TORCH_CHECK(max_seg >= 1 && max_seg <= 64, "aiko.voice_activity_out: 1 <= max_seg <= 64 required, got ", max_seg);
  for (const at::Tensor* t : {&count, &speech, &silent})
    TORCH_CHECK(t->scalar_type() == at::kInt && t->dim() == 1 && t->size(0) == B && t->is_contiguous(),
                "aiko.voice_activity_out: count, speech and silent int32 [B] contiguous required");
  // no output may overlap an input or another output
  auto overlap = [](const at::Tensor& x, const at::Tensor& y) {
    const auto xp = reinterpret_cast<uintptr_t>(x.data_ptr()), yp = reinterpret_cast<uintptr_t>(y.data_ptr());
    const uintptr_t xn = x.numel() * x.element_size(), yn = y.numel() * y.element_size();
    return xn > 0 && yn > 0 && xp < yp + yn && yp < xp + xn;
  };
  for (int o = 0; o < 8; ++o) {
    for (int i = 0; i < 2; ++i)
      TORCH_CHECK(!overlap(*outs[o], *ins[i]), "aiko.voice_activity_out: ", out_names[o], " and ", in_names[i],
                  " overlap");
    for (int p = 0; p < o; ++p)
      TORCH_CHECK(!overlap(*outs[o], *outs[p]), "aiko.voice_activity_out: ", out_names[o], " and ", out_names[p],
                  " overlap");
  }
  check_launch(aiko_voice_activity(audio.data_ptr<float>(), state.data_ptr<int>(), state_out.data_ptr<int>(),
                                   level.data_ptr<int>(), zc.data_ptr<int>(), mask.data_ptr(), seg.data_ptr<int>(),
                                   count.data_ptr<int>(), speech.data_ptr<int>(), silent.data_ptr<int>(), (int)B, (int)F,
                                   (int)frame, (int)threshold, (int)min_level, (int)up_shift, (int)speech_shift,
                                   (int)down_shift, (int)warmup, (int)attack, (int)hang, (int)max_zc, (int)window,
                                   (int)max_seg, cur_stream()),
               "voice_activity");
}

// One spectrum step (spectrum_ops.hip; the rule is in ops/spectrum.py): audio fp32 [B, n] and the host tables
// window [n_fft], twiddle [n_fft / 2, 2], band_start [bands + 1] -> power [B, F, K], amplitudes [B, K],
// band_amplitudes [B, bands], peak_bins / peak_amplitudes [B, max_peaks], peak_counts [B].  inv_F, lo and hi are
// fp32 values.  Two launches on the current stream
void spectrum_out(const at::Tensor& audio, const at::Tensor& window, const at::Tensor& twiddle,
                  const at::Tensor& band_start, int64_t n_fft, int64_t hop, double inv_F, double lo, double hi,
                  int64_t k_lo, int64_t k_hi, bool local, at::Tensor& power, at::Tensor& amplitudes,
                  at::Tensor& band_amplitudes, at::Tensor& peak_bins, at::Tensor& peak_amplitudes,
                  at::Tensor& peak_counts) {
  const at::Tensor* ins[4] = {&audio, &window, &twiddle, &band_start};
  const char* in_names[4] = {"audio", "window", "twiddle", "band_start"};
  const at::Tensor* outs[6] = {&power, &amplitudes, &band_amplitudes, &peak_bins, &peak_amplitudes, &peak_counts};
  const char* out_names[6] = {"power", "amplitudes", "band_amplitudes", "peak_bins", "peak_amplitudes", "peak_counts"};
  for (int i = 0; i < 4; ++i) check_cuda(*ins[i], in_names[i]);
  for (int o = 0; o < 6; ++o) check_cuda(*outs[o], out_names[o]);
  for (int i = 1; i < 4; ++i)
    TORCH_CHECK(ins[i]->device() == audio.device(), "aiko.spectrum_out: tensors on different devices");
  for (int o = 0; o < 6; ++o)
    TORCH_CHECK(outs[o]->device() == audio.device(), "aiko.spectrum_out: tensors on different devices");
  TORCH_CHECK(audio.scalar_type() == at::kFloat && audio.dim() == 2 && audio.is_contiguous() && audio.size(0) >= 1 &&
                  audio.size(1) >= 1,
              "aiko.spectrum_out: audio fp32 [B, n >= 1] contiguous required");
  TORCH_CHECK(n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096 || n_fft == 8192,
              "aiko.spectrum_out: n_fft in {256, 512, 1024, 2048, 4096, 8192} required, got ", n_fft);
  TORCH_CHECK(hop >= 1 && hop <= n_fft, "aiko.spectrum_out: 1 <= hop <= n_fft required, got ", hop);
  const int64_t B = audio.size(0), n = audio.size(1), K = n_fft / 2 + 1;
  TORCH_CHECK(n <= INT_MAX, "aiko.spectrum_out: n = ", n, " exceeds 2^31 - 1 samples");
  const int64_t F = n < n_fft ? 1 : 1 + (n - n_fft) / hop;
  TORCH_CHECK(F <= 4096, "aiko.spectrum_out: F = ", F, " frames exceed 4096 per call");
  TORCH_CHECK(B <= 65535, "aiko.spectrum_out: B = ", B, " exceeds the grid limit (65535 streams)");
  auto is_f32 = [](const at::Tensor& t, std::initializer_list<int64_t> shape) {
    return t.scalar_type() == at::kFloat && t.is_contiguous() && t.sizes() == at::IntArrayRef(shape);
  };
  TORCH_CHECK(is_f32(window, {n_fft}), "aiko.spectrum_out: window fp32 [n_fft = ", n_fft, "] contiguous required");
  TORCH_CHECK(is_f32(twiddle, {n_fft / 2, 2}), "aiko.spectrum_out: twiddle fp32 [n_fft / 2 = ", n_fft / 2,
              ", 2] contiguous required");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(twiddle.data_ptr()) % 8 == 0, "aiko.spectrum_out: twiddle 8-byte aligned "
              "required");
  TORCH_CHECK(band_start.scalar_type() == at::kInt && band_start.dim() == 1 && band_start.is_contiguous() &&
                  band_start.size(0) >= 2 && band_start.size(0) <= 65,
              "aiko.spectrum_out: band_start int32 [bands + 1], 1 <= bands <= 64, contiguous required");
  const int64_t bands = band_start.size(0) - 1;
  TORCH_CHECK(std::isfinite(inv_F) && std::isfinite(lo) && std::isfinite(hi) && (double)(float)inv_F == inv_F &&
                  (double)(float)lo == lo && (double)(float)hi == hi,
              "aiko.spectrum_out: inv_F, lo and hi finite fp32 values required");
  TORCH_CHECK(k_lo >= 0 && k_lo <= INT_MAX && k_hi >= -1 && k_hi <= INT_MAX,
              "aiko.spectrum_out: k_lo >= 0 and k_hi >= -1 required, got ", k_lo, ", ", k_hi);
  TORCH_CHECK(is_f32(power, {B, F, K}), "aiko.spectrum_out: power fp32 [B, F, K] = [", B, ", ", F, ", ", K,
              "] contiguous required");
  TORCH_CHECK(is_f32(amplitudes, {B, K}), "aiko.spectrum_out: amplitudes fp32 [B, K] = [", B, ", ", K,
              "] contiguous required");
  TORCH_CHECK(is_f32(band_amplitudes, {B, bands}), "aiko.spectrum_out: band_amplitudes fp32 [B, bands] = [", B, ", ",
              bands, "] contiguous required");
  TORCH_CHECK(peak_bins.scalar_type() == at::kInt && peak_bins.dim() == 2 && peak_bins.size(0) == B &&
                  peak_bins.is_contiguous(),
              "aiko.spectrum_out: peak_bins int32 [B, max_peaks] contiguous required");
  const int64_t max_peaks = peak_bins.size(1);
  TORCH_CHECK(max_peaks >= 1 && max_peaks <= 128, "aiko.spectrum_out: 1 <= max_peaks <= 128 required, got ",
              max_peaks);
  TORCH_CHECK(is_f32(peak_amplitudes, {B, max_peaks}), "aiko.spectrum_out: peak_amplitudes fp32 [B, max_peaks] = [", B,
              ", ", max_peaks, "] contiguous required");
  TORCH_CHECK(peak_counts.scalar_type() == at::kInt && peak_counts.dim() == 1 && peak_counts.size(0) == B &&
                  peak_counts.is_contiguous(),
              "aiko.spectrum_out: peak_counts int32 [B] contiguous required");
  // no output may overlap an input or another output
  auto overlap = [](const at::Tensor& x, const at::Tensor& y) {
    const auto xp = reinterpret_cast<uintptr_t>(x.data_ptr()), yp = reinterpret_cast<uintptr_t>(y.data_ptr());
    const uintptr_t xn = x.numel() * x.element_size(), yn = y.numel() * y.element_size();
    return xn > 0 && yn > 0 && xp < yp + yn && yp < xp + xn;
  };
  for (int o = 0; o < 6; ++o) {
    for (int i = 0; i < 4; ++i)
      TORCH_CHECK(!overlap(*outs[o], *ins[i]), "aiko.spectrum_out: ", out_names[o], " and ", in_names[i], " overlap");
    for (int p = 0; p < o; ++p)
      TORCH_CHECK(!overlap(*outs[o], *outs[p]), "aiko.spectrum_out: ", out_names[o], " and ", out_names[p],
                  " overlap");
  }
  check_launch(aiko_spectrum(audio.data_ptr<float>(), window.data_ptr<float>(), twiddle.data_ptr<float>(),
                             band_start.data_ptr<int>(), power.data_ptr<float>(), amplitudes.data_ptr<float>(),
                             band_amplitudes.data_ptr<float>(), peak_bins.data_ptr<int>(),
                             peak_amplitudes.data_ptr<float>(), peak_counts.data_ptr<int>(), (int)B, (long)n, (int)F,
                             (int)n_fft, (int)hop, (int)bands, (int)max_peaks, (float)inv_F, (float)lo, (float)hi,
                             (int)k_lo, (int)k_hi, local ? 1 : 0, cur_stream()),
               "spectrum");
}

// The scatter graph of a spectrum's peaks (spectrum_ops.hip; step 8 of the rule in ops/spectrum.py): peak_bins /
// peak_amplitudes [B, max_peaks], peak_counts [B] and bin_px int32 [K] -> image uint8 [B, H, W, 3].  One launch
void spectrum_graph_out(const at::Tensor& peak_bins, const at::Tensor& peak_amplitudes, const at::Tensor& peak_counts,
                        const at::Tensor& bin_px, double y_max, at::IntArrayRef color, at::Tensor& image) {
  const at::Tensor* ts[5] = {&peak_bins, &peak_amplitudes, &peak_counts, &bin_px, &image};
  const char* names[5] = {"peak_bins", "peak_amplitudes", "peak_counts", "bin_px", "image"};
  for (int i = 0; i < 5; ++i) check_cuda(*ts[i], names[i]);
  for (int i = 1; i < 5; ++i)
    TORCH_CHECK(ts[i]->device() == peak_bins.device(), "aiko.spectrum_graph_out: tensors on different devices");
  TORCH_CHECK(peak_bins.scalar_type() == at::kInt && peak_bins.dim() == 2 && peak_bins.is_contiguous() &&
                  peak_bins.size(0) >= 1,
              "aiko.spectrum_graph_out: peak_bins int32 [B, max_peaks] contiguous required");
  const int64_t B = peak_bins.size(0), max_peaks = peak_bins.size(1);
  TORCH_CHECK(max_peaks >= 1 && max_peaks <= 128, "aiko.spectrum_graph_out: 1 <= max_peaks <= 128 required, got ",
              max_peaks);
  TORCH_CHECK(B <= 65535, "aiko.spectrum_graph_out: B = ", B, " exceeds the grid limit (65535 streams)");
  TORCH_CHECK(peak_amplitudes.scalar_type() == at::kFloat && peak_amplitudes.is_contiguous() &&
                  peak_amplitudes.sizes() == peak_bins.sizes(),
              "aiko.spectrum_graph_out: peak_amplitudes fp32 [B, max_peaks] = [", B, ", ", max_peaks,
              "] contiguous required");
  TORCH_CHECK(peak_counts.scalar_type() == at::kInt && peak_counts.dim() == 1 && peak_counts.size(0) == B &&
                  peak_counts.is_contiguous(),
              "aiko.spectrum_graph_out: peak_counts int32 [B] contiguous required");
  TORCH_CHECK(bin_px.scalar_type() == at::kInt && bin_px.dim() == 1 && bin_px.size(0) >= 1 &&
                  bin_px.size(0) <= 4097 && bin_px.is_contiguous(),
              "aiko.spectrum_graph_out: bin_px int32 [K <= 4097] contiguous required");
  TORCH_CHECK(image.scalar_type() == at::kByte && image.dim() == 4 && image.size(0) == B && image.size(3) == 3 &&
                  image.is_contiguous(),
              "aiko.spectrum_graph_out: image uint8 [B, H, W, 3] contiguous required, B = ", B);
  const int64_t H = image.size(1), W = image.size(2);
  TORCH_CHECK(H >= 16 && H <= 4096 && W >= 16 && W <= 4096,
              "aiko.spectrum_graph_out: 16 <= H, W <= 4096 required, got ", H, " x ", W);
  TORCH_CHECK(std::isfinite(y_max) && y_max > 0.0, "aiko.spectrum_graph_out: y_max > 0 required, got ", y_max);
  TORCH_CHECK(color.size() == 3, "aiko.spectrum_graph_out: color [r, g, b] required");
  for (int64_t c : color) TORCH_CHECK(c >= 0 && c <= 255, "aiko.spectrum_graph_out: color in 0..255 required, got ", c);
  auto overlap = [](const at::Tensor& x, const at::Tensor& y) {
    const auto xp = reinterpret_cast<uintptr_t>(x.data_ptr()), yp = reinterpret_cast<uintptr_t>(y.data_ptr());
    const uintptr_t xn = x.numel() * x.element_size(), yn = y.numel() * y.element_size();
    return xn > 0 && yn > 0 && xp < yp + yn && yp < xp + xn;
  };
  for (int i = 0; i < 4; ++i)
    TORCH_CHECK(!overlap(image, *ts[i]), "aiko.spectrum_graph_out: image and ", names[i], " overlap");
  check_launch(aiko_spectrum_graph(peak_bins.data_ptr<int>(), peak_amplitudes.data_ptr<float>(),
                                   peak_counts.data_ptr<int>(), bin_px.data_ptr<int>(), image.data_ptr(), (int)B, (int)H,
                                   (int)W, (int)bin_px.size(0), (int)max_peaks, y_max, (int)color[0], (int)color[1],
                                   (int)color[2], cur_stream()),
               "spectrum_graph");
}

// Baseline JPEG (jpeg_ops.hip; the rule is in ops/jpeg.py): raw planar frames [B, frame_bytes] (fmt 1: i420,
// 2: i444) -> one JFIF stream per frame in stream [B, cap], its length (-1: overflow) in nbytes [B].  tables is
// ops.jpeg.device_tables' tensor (864 words, then header_len bytes of header); workspace holds an int32 and
// seg_cap bytes per (frame, MCU row).  Two launches on the current stream
void jpeg_encode_out(const at::Tensor& raw, int64_t height, int64_t width, int64_t fmt, const at::Tensor& tables,
                     int64_t header_len, int64_t seg_cap, at::Tensor& stream, at::Tensor& nbytes,
                     at::Tensor& workspace) {
  const at::Tensor* ts[5] = {&raw, &tables, &stream, &nbytes, &workspace};
  const char* names[5] = {"raw", "tables", "stream", "nbytes", "workspace"};
  for (int i = 0; i < 5; ++i) check_cuda(*ts[i], names[i]);
  for (int i = 1; i < 5; ++i)
    TORCH_CHECK(ts[i]->device() == raw.device(), "aiko.jpeg_encode_out: tensors on different devices");
  TORCH_CHECK(fmt == 1 || fmt == 2, "aiko.jpeg_encode_out: fmt 1 (i420) or 2 (i444) required, got ", fmt);
  TORCH_CHECK(height >= 1 && height <= 65535 && width >= 1 && width <= 4096,
              "aiko.jpeg_encode_out: 1 <= height <= 65535 and 1 <= width <= 4096 required, got ", height, " x ", width);
  const int64_t H = height, W = width, mcu = fmt == 1 ? 16 : 8;
  const int64_t my = (H + mcu - 1) / mcu;
  const int64_t frame = fmt == 1 ? H * W + 2 * ((H + 1) / 2) * ((W + 1) / 2) : 3 * H * W;
  TORCH_CHECK(raw.scalar_type() == at::kByte && raw.dim() == 2 && raw.size(1) == frame && raw.is_contiguous() &&
                  raw.size(0) >= 1,
              "aiko.jpeg_encode_out: raw uint8 [B, ", frame, "] contiguous required");
  const int64_t B = raw.size(0);
  TORCH_CHECK(B <= 65535, "aiko.jpeg_encode_out: B = ", B, " exceeds the grid limit (65535 frames)");
  TORCH_CHECK(seg_cap >= 1 && seg_cap <= 96 * 1024, "aiko.jpeg_encode_out: 1 <= seg_cap <= 98304 required, got ",
              seg_cap);
  TORCH_CHECK(header_len >= 1 && tables.scalar_type() == at::kByte && tables.dim() == 1 && tables.is_contiguous() &&
                  tables.numel() == 4 * 864 + header_len && reinterpret_cast<uintptr_t>(tables.data_ptr()) % 4 == 0,
              "aiko.jpeg_encode_out: tables uint8 [3456 + header_len] contiguous, 4-byte aligned required");
  TORCH_CHECK(stream.scalar_type() == at::kByte && stream.dim() == 2 && stream.size(0) == B && stream.size(1) >= 1 &&
                  stream.size(1) <= INT_MAX && stream.is_contiguous(),
              "aiko.jpeg_encode_out: stream uint8 [B, cap] contiguous required, 1 <= cap < 2^31");
  TORCH_CHECK(nbytes.scalar_type() == at::kInt && nbytes.dim() == 1 && nbytes.size(0) == B && nbytes.is_contiguous(),
              "aiko.jpeg_encode_out: nbytes int32 [B] contiguous required");
  const int64_t need = B * my * (4 + seg_cap);
  TORCH_CHECK(workspace.scalar_type() == at::kByte && workspace.dim() == 1 && workspace.is_contiguous() &&
                  workspace.numel() >= need && reinterpret_cast<uintptr_t>(workspace.data_ptr()) % 4 == 0,
              "aiko.jpeg_encode_out: workspace uint8 [>= ", need, "] contiguous, 4-byte aligned required");
  // no output may overlap an input or another output
  auto overlap = [](const at::Tensor& x, const at::Tensor& y) {
    const auto xp = reinterpret_cast<uintptr_t>(x.data_ptr()), yp = reinterpret_cast<uintptr_t>(y.data_ptr());
    const uintptr_t xn = x.numel() * x.element_size(), yn = y.numel() * y.element_size();
    return xn > 0 && yn > 0 && xp < yp + yn && yp < xp + xn;
  };
  for (int o = 2; o < 5; ++o)
    for (int p = 0; p < o; ++p)
      TORCH_CHECK(!overlap(*ts[o], *ts[p]), "aiko.jpeg_encode_out: ", names[o], " and ", names[p], " overlap");
  check_launch(aiko_jpeg_encode(raw.data_ptr(), tables.data_ptr(), (int)header_len, workspace.data_ptr(),
                                stream.data_ptr(), nbytes.data_ptr<int>(), (int)B, (int)H, (int)W, (int)fmt,
                                (long)stream.size(1), (int)seg_cap, cur_stream()),
               "jpeg_encode");
}

// Baseline JPEG decoding (jpeg_decode_ops.hip; the rule, the descriptor and the workspace are in
// ops/jpeg_decode.py): one stream per row of data [B, cap], its length in nbytes [B], its header's descriptor
// in desc [B, 1744] or [1, 1744] (one for all) -> raw frames [B, frame_bytes] (fmt 1: i420, 2: i444, 3: yuyv) and
// a status per frame.  max_intervals: the restart intervals per frame provided for.  Three launches on the
// current stream
void jpeg_decode_out(const at::Tensor& data, const at::Tensor& nbytes, const at::Tensor& desc, int64_t height,
                     int64_t width, int64_t fmt, int64_t max_intervals, at::Tensor& raw, at::Tensor& status,
                     at::Tensor& workspace) {
  const at::Tensor* ts[6] = {&data, &nbytes, &desc, &raw, &status, &workspace};
  const char* names[6] = {"data", "nbytes", "desc", "raw", "status", "workspace"};
  for (int i = 0; i < 6; ++i) check_cuda(*ts[i], names[i]);
  for (int i = 1; i < 6; ++i)
    TORCH_CHECK(ts[i]->device() == data.device(), "aiko.jpeg_decode_out: tensors on different devices");
  TORCH_CHECK(fmt == 1 || fmt == 2 || fmt == 3, "aiko.jpeg_decode_out: fmt 1 (i420), 2 (i444) or 3 (yuyv) required, got ",
              fmt);
  TORCH_CHECK(height >= 1 && height <= 65535 && width >= 1 && width <= 4096,
              "aiko.jpeg_decode_out: 1 <= height <= 65535 and 1 <= width <= 4096 required, got ", height, " x ", width);
  TORCH_CHECK(fmt != 3 || width % 2 == 0, "aiko.jpeg_decode_out: yuyv needs an even width, got ", width);
  const int64_t H = height, W = width, mh = fmt == 1 ? 16 : 8, mw = fmt == 2 ? 8 : 16;
  const int64_t mcus = ((H + mh - 1) / mh) * ((W + mw - 1) / mw);
  const int64_t nblocks = mcus * (fmt == 1 ? 6 : (fmt == 2 ? 3 : 4));
  const int64_t frame = fmt == 1 ? H * W + 2 * ((H + 1) / 2) * ((W + 1) / 2) : (fmt == 2 ? 3 * H * W : 2 * H * W);
  TORCH_CHECK(max_intervals >= 1 && max_intervals <= mcus, "aiko.jpeg_decode_out: 1 <= max_intervals <= ", mcus,
              " (the frame's MCUs) required, got ", max_intervals);
  TORCH_CHECK(data.scalar_type() == at::kByte && data.dim() == 2 && data.size(0) >= 1 && data.size(1) >= 1 &&
                  data.size(1) <= INT_MAX && data.is_contiguous(),
              "aiko.jpeg_decode_out: data uint8 [B, cap] contiguous required, 1 <= cap < 2^31");
  const int64_t B = data.size(0);
  TORCH_CHECK(B <= 65535, "aiko.jpeg_decode_out: B = ", B, " exceeds the grid limit (65535 frames)");
  TORCH_CHECK(nbytes.scalar_type() == at::kInt && nbytes.dim() == 1 && nbytes.size(0) == B && nbytes.is_contiguous(),
              "aiko.jpeg_decode_out: nbytes int32 [B] contiguous required");
  TORCH_CHECK(desc.scalar_type() == at::kByte && desc.dim() == 2 && (desc.size(0) == B || desc.size(0) == 1) &&
                  desc.size(1) == 1744 && desc.is_contiguous() && reinterpret_cast<uintptr_t>(desc.data_ptr()) % 4 == 0,
              "aiko.jpeg_decode_out: desc uint8 [B, 1744] or [1, 1744] contiguous, 4-byte aligned required");
  TORCH_CHECK(raw.scalar_type() == at::kByte && raw.dim() == 2 && raw.size(0) == B && raw.size(1) == frame &&
                  raw.is_contiguous(),
              "aiko.jpeg_decode_out: raw uint8 [B, ", frame, "] contiguous required");
  TORCH_CHECK(status.scalar_type() == at::kInt && status.dim() == 1 && status.size(0) == B && status.is_contiguous(),
              "aiko.jpeg_decode_out: status int32 [B] contiguous required");
  const int64_t need = (4 * B * (1 + 2 * max_intervals) + 15) / 16 * 16 + B * nblocks * 128;
  TORCH_CHECK(workspace.scalar_type() == at::kByte && workspace.dim() == 1 && workspace.is_contiguous() &&
                  workspace.numel() >= need && reinterpret_cast<uintptr_t>(workspace.data_ptr()) % 16 == 0,
              "aiko.jpeg_decode_out: workspace uint8 [>= ", need, "] contiguous, 16-byte aligned required");
  // no output may overlap an input or another output
  auto overlap = [](const at::Tensor& x, const at::Tensor& y) {
    const auto xp = reinterpret_cast<uintptr_t>(x.data_ptr()), yp = reinterpret_cast<uintptr_t>(y.data_ptr());
    const uintptr_t xn = x.numel() * x.element_size(), yn = y.numel() * y.element_size();
    return xn > 0 && yn > 0 && xp < yp + yn && yp < xp + xn;
  };
  for (int o = 3; o < 6; ++o)
    for (int p = 0; p < o; ++p)
      TORCH_CHECK(!overlap(*ts[o], *ts[p]), "aiko.jpeg_decode_out: ", names[o], " and ", names[p], " overlap");
  check_launch(aiko_jpeg_decode(data.data_ptr(), nbytes.data_ptr<int>(), desc.data_ptr(), (int)desc.size(0),
                                workspace.data_ptr(), raw.data_ptr(), status.data_ptr<int>(), (int)B, (int)H, (int)W,
                                (int)fmt, (long)data.size(1), (int)max_intervals, cur_stream()),
               "jpeg_decode");
}

void avgpool_out(const at::Tensor& x, at::Tensor& y) {
  check_cuda(x, "x");
  check_cuda(y, "y");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && y.scalar_type() == at::kBFloat16 &&
                  x.dim() == 4 && x.is_contiguous() && y.is_contiguous(),
              "aiko.avgpool_out: NHWC bf16 contiguous tensors required");
  const int64_t B = x.size(0), C = x.size(3);
  TORCH_CHECK(C % 8 == 0 && y.numel() == B * C, "aiko.avgpool_out: bad shapes");
  check_launch(aiko_avgpool(x.data_ptr(), y.data_ptr(), B, x.size(1) * x.size(2), C, cur_stream()),
               "avgpool");
}

void softmax_topk_out(const at::Tensor& logits, at::Tensor& prob, at::Tensor& index, int64_t k) {
  check_cuda(logits, "logits");
  check_cuda(prob, "prob");
  check_cuda(index, "index");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 && logits.dim() == 2 && logits.is_contiguous(),
              "aiko.softmax_topk_out: logits must be bf16 [B, N] contiguous");
  TORCH_CHECK(prob.scalar_type() == at::kFloat && index.scalar_type() == at::kInt,
              "aiko.softmax_topk_out: prob fp32, index int32");
  const int64_t B = logits.size(0), N = logits.size(1);
  TORCH_CHECK(k >= 1 && k <= 8 && k <= N, "aiko.softmax_topk_out: 1 <= k <= min(8, N)");
  TORCH_CHECK(prob.numel() == B * k && index.numel() == B * k, "aiko.softmax_topk_out: outputs must hold B*k");
  check_launch(aiko_softmax_topk(logits.data_ptr(), prob.data_ptr<float>(), index.data_ptr<int>(),
                                 B, N, k, cur_stream()),
               "softmax_topk");
}

// ---- transformer / fp8 ------------------------------------------------------------------------

int64_t row_pitch(const at::Tensor& t, int64_t cols, const char* op, const char* name) {
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1 && t.size(1) == cols && t.stride(0) >= cols,
              "aiko.", op, ": ", name, " must be a row-major [rows, ", cols, "] matrix (row slices / column slices allowed)");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 && (t.stride(0) * t.element_size()) % 16 == 0,
              "aiko.", op, ": ", name, " rows must be 16-byte aligned");
  TORCH_CHECK(avail_elems(t) >= (t.size(0) - 1) * t.stride(0) + cols, "aiko.", op, ": ", name, " storage too small");
  return t.stride(0);
}

// y = act(sa[m] * sb[n] * (A @ B^T) + bias) + residual ; A fp8 [M, K] (uint8 storage), B fp8 [N, K].
// MX-fp8 options (LDS-DMA kernel, variant 1): ``amx`` uint8 [K/128, R, 4] E8M0 block scales of A
// (replaces ``sa``); ``yq`` uint8 [M, N] + ``ysc`` uint8 [N/128, R2, 4]: quantise the output to
// MX-fp8 instead of writing bf16 ``y`` (then ``y`` may be omitted).
void gemm_fp8_out(const at::Tensor& a, const c10::optional<at::Tensor>& sa_opt, const at::Tensor& b,
                  const at::Tensor& sb, const c10::optional<at::Tensor>& bias,
                  const c10::optional<at::Tensor>& res, const c10::optional<at::Tensor>& y_opt, int64_t act,
                  int64_t bm, int64_t bn, int64_t variant, const c10::optional<at::Tensor>& zero,
                  const c10::optional<at::Tensor>& amx, const c10::optional<at::Tensor>& yq,
                  const c10::optional<at::Tensor>& ysc) {
  for (const at::Tensor* t : {&a, &b, &sb}) check_cuda(*t, "operand");
  TORCH_CHECK(a.element_size() == 1 && b.element_size() == 1, "aiko.gemm_fp8_out: A and B must be 1-byte fp8 storage");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(K % 128 == 0 && b.dim() == 2 && b.size(1) == K && b.is_contiguous(),
              "aiko.gemm_fp8_out: K must be a multiple of 128 and B [N, K] contiguous");
  TORCH_CHECK(N % 8 == 0, "aiko.gemm_fp8_out: N must be a multiple of 8");
  const int64_t lda = row_pitch(a, K, "gemm_fp8_out", "A");
  TORCH_CHECK(sb.scalar_type() == at::kFloat && sb.numel() == N && sb.is_contiguous(), "aiko.gemm_fp8_out: sb fp32 [N]");
  const bool mx_in = amx.has_value() && amx->defined();
  const bool mx_out = yq.has_value() && yq->defined();
  const float* sap = nullptr;
  if (!mx_in) {
    TORCH_CHECK(sa_opt.has_value() && sa_opt->defined(), "aiko.gemm_fp8_out: sa needed without amx");
    const at::Tensor& sa = *sa_opt;
    check_cuda(sa, "sa");
    TORCH_CHECK(sa.scalar_type() == at::kFloat && sa.numel() >= M && sa.is_contiguous(), "aiko.gemm_fp8_out: sa fp32 [M]");
    sap = sa.data_ptr<float>();
  }
  const void* amxp = nullptr;
  int64_t mxr = 0;
  if (mx_in) {
    check_cuda(*amx, "amx");
    TORCH_CHECK(amx->element_size() == 1 && amx->dim() == 3 && amx->size(0) == K / 128 && amx->size(2) == 4 &&
                    amx->is_contiguous() && amx->size(1) >= ((M + 127) / 128) * 128,
                "aiko.gemm_fp8_out: amx must be uint8 [K/128, rows >= M rounded to 128, 4]");
    amxp = amx->data_ptr();
    mxr = amx->size(1);
  }
  void* yp = nullptr;
  int64_t ldy = 0;
  if (y_opt.has_value() && y_opt->defined()) {
    check_cuda(*y_opt, "y");
    TORCH_CHECK(y_opt->scalar_type() == at::kBFloat16 && y_opt->size(0) == M, "aiko.gemm_fp8_out: y must be bf16 [M, N]");
    ldy = row_pitch(*y_opt, N, "gemm_fp8_out", "y");
    yp = y_opt->data_ptr();
  }
  void* yqp = nullptr;
  void* yscp = nullptr;
  int64_t ldq = 0, ysr = 0;
  if (mx_out) {
    check_cuda(*yq, "yq");
    TORCH_CHECK(ysc.has_value() && ysc->defined(), "aiko.gemm_fp8_out: yq needs ysc");
    check_cuda(*ysc, "ysc");
    TORCH_CHECK(yq->element_size() == 1 && yq->size(0) == M && N % 128 == 0, "aiko.gemm_fp8_out: yq uint8 [M, N], N % 128 == 0");
    ldq = row_pitch(*yq, N, "gemm_fp8_out", "yq");
    TORCH_CHECK(ysc->element_size() == 1 && ysc->dim() == 3 && ysc->size(0) == N / 128 && ysc->size(1) >= M &&
                    ysc->size(2) == 4 && ysc->is_contiguous(),
                "aiko.gemm_fp8_out: ysc must be uint8 [N/128, rows >= M, 4]");
    TORCH_CHECK(!(res.has_value() && res->defined()), "aiko.gemm_fp8_out: no residual with MX output");
    yqp = yq->data_ptr();
    yscp = ysc->data_ptr();
    ysr = ysc->size(1);
  } else {
    TORCH_CHECK(yp != nullptr, "aiko.gemm_fp8_out: y (or yq) required");
  }
  TORCH_CHECK(!(mx_in || mx_out) || (variant == 1 && bn == 128) || (variant == 3 && bm == 256 && bn == 256 && N % 256 == 0) ||
                  (variant == 4 && bm == 256 && bn == 256 && N % 256 == 0) ||
                  (variant == 5 && bm == 128 && bn == 256 && N % 256 == 0),
              "aiko.gemm_fp8_out: MX paths need variant 1 with BN 128, variant 3 (256 x 256, N % 256 == 0), "
              "variant 4 (persistent 256 x 256) or variant 5 (persistent 128 x 256)");
  const float* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == N && bias->is_contiguous(), "aiko.gemm_fp8_out: bias fp32 [N]");
    bp = bias->data_ptr<float>();
  }
  const void* rp = nullptr;
  int64_t ldr = 0;
  if (res.has_value() && res->defined()) {
    check_cuda(*res, "residual");
    TORCH_CHECK(res->scalar_type() == at::kBFloat16 && res->size(0) == M, "aiko.gemm_fp8_out: residual bf16 [M, N]");
    ldr = row_pitch(*res, N, "gemm_fp8_out", "residual");
    rp = res->data_ptr();
  }
  TORCH_CHECK(lda * M < INT_MAX * 2L, "aiko.gemm_fp8_out: A too large");
  const void* zp = nullptr;
  if (variant >= 1) {
    TORCH_CHECK(zero.has_value() && zero->defined() && zero->is_cuda() && zero->nbytes() >= 16 &&
                    reinterpret_cast<uintptr_t>(zero->data_ptr()) % 16 == 0,
                "aiko.gemm_fp8_out: the LDS-DMA variants need a zero page tensor (>= 16 B)");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(b.data_ptr()) % 16 == 0,
                "aiko.gemm_fp8_out: operands must be 16-byte aligned");
    zp = zero->data_ptr();
  }
  check_launch(aiko_gemm_fp8(a.data_ptr(), b.data_ptr(), sap, sb.data_ptr<float>(), bp, rp, yp, M, N, K, lda,
                             ldy, ldr, act, bm, bn, (int)variant, zp, amxp, (int)mxr, yqp, yscp, (int)ldq,
                             (int)ysr, cur_stream()),
               "gemm_fp8");
}

// LayerNorm (gamma/beta given) and/or per-row fp8 quantisation of bf16 rows x [M, D]
void rownorm_quant_out(const at::Tensor& x, const c10::optional<at::Tensor>& gamma,
                       const c10::optional<at::Tensor>& beta, double eps,
                       const c10::optional<at::Tensor>& yb, const c10::optional<at::Tensor>& q,
                       const c10::optional<at::Tensor>& qs) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "aiko.rownorm_quant_out: x must be bf16");
  const int64_t M = x.size(0), D = x.size(1);
  TORCH_CHECK(D % 8 == 0 && D <= 8192, "aiko.rownorm_quant_out: D % 8 == 0, D <= 8192");
  const int64_t ldx = row_pitch(x, D, "rownorm_quant_out", "x");
  const float *g = nullptr, *be = nullptr;
  if (gamma.has_value() && gamma->defined()) {
    TORCH_CHECK(beta.has_value() && beta->defined(), "aiko.rownorm_quant_out: gamma needs beta");
    check_cuda(*gamma, "gamma");
    check_cuda(*beta, "beta");
    TORCH_CHECK(gamma->scalar_type() == at::kFloat && beta->scalar_type() == at::kFloat && gamma->numel() == D &&
                    beta->numel() == D && gamma->is_contiguous() && beta->is_contiguous(),
                "aiko.rownorm_quant_out: gamma/beta fp32 [D]");
    g = gamma->data_ptr<float>();
    be = beta->data_ptr<float>();
  }
  void* yp = nullptr;
  int64_t ldyb = 0;
  if (yb.has_value() && yb->defined()) {
    check_cuda(*yb, "yb");
    TORCH_CHECK(yb->scalar_type() == at::kBFloat16 && yb->size(0) == M, "aiko.rownorm_quant_out: yb bf16 [M, D]");
    ldyb = row_pitch(*yb, D, "rownorm_quant_out", "yb");
    yp = yb->data_ptr();
  }
  void* qp = nullptr;
  float* sp = nullptr;
  int64_t ldq = 0;
  if (q.has_value() && q->defined()) {
    TORCH_CHECK(qs.has_value() && qs->defined(), "aiko.rownorm_quant_out: q needs qs");
    check_cuda(*q, "q");
    check_cuda(*qs, "qs");
    TORCH_CHECK(q->element_size() == 1 && q->size(0) == M, "aiko.rownorm_quant_out: q fp8 [M, D]");
    ldq = row_pitch(*q, D, "rownorm_quant_out", "q");
    TORCH_CHECK(qs->scalar_type() == at::kFloat && qs->numel() >= M && qs->is_contiguous(), "aiko.rownorm_quant_out: qs fp32 [M]");
    qp = q->data_ptr();
    sp = qs->data_ptr<float>();
  }
  TORCH_CHECK(yp || qp, "aiko.rownorm_quant_out: nothing to write");
  check_launch(aiko_rownorm_quant(x.data_ptr(), ldx, g, be, (float)eps, yp, ldyb, qp, ldq, sp, M, D, cur_stream()),
               "rownorm_quant");
}



// Split-K linear (linear_splitk.hip): x [M, >= K] bf16, w [N, >= K] bf16 (row pitch w.stride(0)),
// bias fp32 [N] or None, part fp32 with >= S*M*N elements, y [M, >= N] bf16.
void linear_splitk_out(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                       at::Tensor& part, at::Tensor& y, int64_t K, int64_t S) {
  for (const at::Tensor* t : {&x, &w, (const at::Tensor*)&part, (const at::Tensor*)&y}) check_cuda(*t, "x/w/part/y");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16 && y.scalar_type() == at::kBFloat16,
              "aiko.linear_splitk_out: x, w, y must be bf16");
  TORCH_CHECK(part.scalar_type() == at::kFloat && part.is_contiguous(), "aiko.linear_splitk_out: part must be contiguous fp32");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && y.dim() == 2 && x.stride(1) == 1 && w.stride(1) == 1 && y.stride(1) == 1,
              "aiko.linear_splitk_out: row-major 2-D operands");
  const int64_t M = x.size(0), N = w.size(0);
  TORCH_CHECK(y.size(0) == M && y.size(1) == N && x.size(1) >= K && w.size(1) >= K, "aiko.linear_splitk_out: shapes");
  TORCH_CHECK(S >= 1 && K % (32 * S) == 0 && N % 4 == 0, "aiko.linear_splitk_out: K % (32 S) == 0 and N % 4 == 0");
  TORCH_CHECK(x.stride(0) % 8 == 0 && w.stride(0) % 8 == 0 && y.stride(0) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(y.data_ptr()) % 8 == 0 && reinterpret_cast<uintptr_t>(part.data_ptr()) % 16 == 0,
              "aiko.linear_splitk_out: 16-B aligned operand rows");
  TORCH_CHECK(part.numel() >= S * M * N, "aiko.linear_splitk_out: part too small");
  const float* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == N && bias->is_contiguous(),
                "aiko.linear_splitk_out: bias must be fp32 [N]");
    bp = bias->data_ptr<float>();
  }
  check_launch(aiko_linear_splitk(x.data_ptr(), w.data_ptr(), bp, part.data_ptr<float>(), y.data_ptr(), (int)M, (int)N,
                                  (int)K, (int)x.stride(0), (int)w.stride(0), (int)y.stride(0), (int)S, cur_stream()),
               "linear_splitk");
}

// q/k/v/o: [B*Tpad, >= H*64] row-major (column slices of a fused QKV buffer allowed)
void attn_fwd_out(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, at::Tensor& o,
                  int64_t B, int64_t H, int64_t T, int64_t Tpad, double scale,
                  const c10::optional<at::Tensor>& work, const c10::optional<at::Tensor>& oq,
                  const c10::optional<at::Tensor>& osc) {
  for (const at::Tensor* t : {&q, &k, &v, (const at::Tensor*)&o}) {
    check_cuda(*t, "q/k/v/o");
    TORCH_CHECK(t->scalar_type() == at::kBFloat16, "aiko.attn_fwd_out: bf16 tensors required");
    TORCH_CHECK(t->size(0) == B * Tpad, "aiko.attn_fwd_out: tensors need B*Tpad rows");
    row_pitch(*t, H * 64, "attn_fwd_out", "q/k/v/o");
  }
  TORCH_CHECK(T >= 1 && T <= Tpad, "aiko.attn_fwd_out: 1 <= T <= Tpad");
  void* wp = nullptr;
  long wb = 0;
  if (work.has_value() && work->defined()) {
    check_cuda(*work, "work");
    TORCH_CHECK(work->is_contiguous() && reinterpret_cast<uintptr_t>(work->data_ptr()) % 256 == 0,
                "aiko.attn_fwd_out: work must be a contiguous, 256-byte aligned (zero-initialised) buffer");
    wp = work->data_ptr();
    wb = (long)(work->numel() * work->element_size());
  }
  // MX-fp8 output (ops.transformer.mx_buffers layout): e4m3 [B*Tpad, >= H*64] + E8M0 scales
  // [H*64/128][rows >= B*Tpad][4]; o is then not written
  void* qp = nullptr;
  void* sp = nullptr;
  int ldoq = 0, osr = 0;
  if (oq.has_value() && oq->defined()) {
    TORCH_CHECK(osc.has_value() && osc->defined(), "aiko.attn_fwd_out: oq needs osc");
    check_cuda(*oq, "oq");
    check_cuda(*osc, "osc");
    TORCH_CHECK(oq->scalar_type() == at::kByte && oq->dim() == 2 && oq->stride(1) == 1 && oq->size(0) == B * Tpad &&
                    oq->size(1) >= H * 64 && oq->stride(0) % 4 == 0,
                "aiko.attn_fwd_out: oq uint8 [B*Tpad, >= H*64] with a 4-byte row pitch");
    TORCH_CHECK((H * 64) % 128 == 0 && osc->scalar_type() == at::kByte && osc->is_contiguous() && osc->dim() == 3 &&
                    osc->size(0) == H * 64 / 128 && osc->size(1) >= B * Tpad && osc->size(2) == 4,
                "aiko.attn_fwd_out: osc uint8 [H*64/128, rows >= B*Tpad, 4]");
    qp = oq->data_ptr();
    sp = osc->data_ptr();
    ldoq = (int)oq->stride(0);
    osr = (int)osc->size(1);
  }
  check_launch(aiko_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), q.stride(0), k.stride(0),
                             v.stride(0), o.stride(0), B, H, T, Tpad, 64, (float)scale, wp, wb, qp, sp, ldoq, osr,
                             cur_stream()),
               "attn_fwd");
}

// audio fp32 [B, N] -> bf16 log-mel rows [B*rows, n_mels] (frame t at row b*rows + pad + t)
void logmel_out(const at::Tensor& audio, const at::Tensor& mel, const at::Tensor& mel_range, int64_t n_fft,
                int64_t hop, int64_t F, at::Tensor& work, at::Tensor& gmax, at::Tensor& dst, int64_t rows,
                int64_t pad) {
  for (const at::Tensor* t : {&audio, &mel, (const at::Tensor*)&work, (const at::Tensor*)&gmax, (const at::Tensor*)&dst})
    check_cuda(*t, "logmel operand");
  TORCH_CHECK(audio.scalar_type() == at::kFloat && audio.dim() == 2 && audio.is_contiguous(), "aiko.logmel_out: audio fp32 [B, N]");
  const int64_t B = audio.size(0), N = audio.size(1), n_mels = mel.size(0);
  TORCH_CHECK(mel.scalar_type() == at::kFloat && mel.is_contiguous() && mel.size(1) == n_fft / 2 + 1,
              "aiko.logmel_out: mel filters fp32 [n_mels, n_fft/2+1]");
  check_cuda(mel_range, "mel_range");
  TORCH_CHECK(mel_range.scalar_type() == at::kInt && mel_range.is_contiguous() && mel_range.numel() == n_mels * 3 &&
                  n_mels <= 128,
              "aiko.logmel_out: mel_range int32 [n_mels, 3] (lo, len, offset), n_mels <= 128");
  TORCH_CHECK(N > n_fft / 2 && F >= 1 && (F - 1) * hop - n_fft / 2 < N, "aiko.logmel_out: bad frame count");
  TORCH_CHECK(work.scalar_type() == at::kFloat && work.numel() >= B * F * n_mels, "aiko.logmel_out: work fp32 [B*F*n_mels]");
  TORCH_CHECK(gmax.scalar_type() == at::kInt && gmax.numel() >= B, "aiko.logmel_out: gmax int32 [B]");
  TORCH_CHECK(dst.scalar_type() == at::kBFloat16 && dst.dim() == 2 && dst.size(1) == n_mels && dst.stride(1) == 1 &&
                  dst.size(0) == B * rows && rows >= F + pad,
              "aiko.logmel_out: dst bf16 [B*rows, n_mels]");
  check_launch(aiko_logmel(audio.data_ptr<float>(), B, N, mel.data_ptr<float>(), n_mels,
                           mel_range.data_ptr<int>(), n_fft, hop, F,
                           work.data_ptr<float>(), gmax.data_ptr<int>(), dst.data_ptr(), rows, pad, dst.stride(0),
                           cur_stream()),
               "logmel");
}

// ---- decoder step ops (decode_ops.hip) ----------------------------------------------------------

void check_i32(const at::Tensor& t, int64_t n, const char* what) {
  check_cuda(t, what);
  TORCH_CHECK(t.scalar_type() == at::kInt && t.is_contiguous() && t.numel() >= n, "aiko: ", what,
              " must be contiguous int32 with >= ", n, " elements");
}

// x[b] = tok[ids[b]] + pemb[pos[0]]; tok bf16 [V, d], pemb bf16 [P, d], x bf16 [B, d]
void embed_tokens_out(const at::Tensor& ids, const at::Tensor& pos, const at::Tensor& tok, const at::Tensor& pemb,
                      at::Tensor& x) {
  const int64_t B = x.size(0), d = x.size(1);
  check_i32(ids, B, "ids");
  check_i32(pos, 1, "pos");
  for (const at::Tensor* t : {&tok, &pemb, (const at::Tensor*)&x}) {
    check_cuda(*t, "embedding operand");
    TORCH_CHECK(t->scalar_type() == at::kBFloat16 && t->dim() == 2 && t->size(1) == d,
                "aiko.embed_tokens_out: bf16 [*, d] tensors required");
  }
  TORCH_CHECK(tok.is_contiguous() && pemb.is_contiguous() && d % 8 == 0, "aiko.embed_tokens_out: contiguous tables, d % 8 == 0");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "aiko.embed_tokens_out: x alignment");
  const int64_t ldx = row_pitch(x, d, "embed_tokens_out", "x");
  check_launch(aiko_embed_tokens(ids.data_ptr<int>(), pos.data_ptr<int>(), tok.data_ptr(), pemb.data_ptr(), x.data_ptr(),
                                 B, d, ldx, tok.size(0), pemb.size(0), cur_stream()),
               "embed_tokens");
}

// One query row per sequence against K/V rows [B*S, >= H*64] (sequence b's key j at row b*S+j).
// With ``pos`` (device int32 [1]) the step appends ``knew``/``vnew`` [B, >= H*64] at row pos of
// every sequence and attends keys 0..pos; otherwise it attends keys 0..T-1.  The kernel reads
// pos on the device: a value < 0 is treated as 0, a value >= S appends nothing and attends the
// S cached keys, so no access leaves the cache.
void attn_decode_out(const at::Tensor& q, at::Tensor& k, at::Tensor& v, at::Tensor& o, int64_t B, int64_t H,
                     int64_t S, int64_t T, const c10::optional<at::Tensor>& pos,
                     const c10::optional<at::Tensor>& knew, const c10::optional<at::Tensor>& vnew, double scale,
                     at::Tensor& work) {
  const bool app = pos.has_value() && pos->defined();
  for (const at::Tensor* t : {&q, (const at::Tensor*)&k, (const at::Tensor*)&v, (const at::Tensor*)&o}) {
    check_cuda(*t, "q/k/v/o");
    TORCH_CHECK(t->scalar_type() == at::kBFloat16 && t->dim() == 2, "aiko.attn_decode_out: bf16 2-D tensors required");
    row_pitch(*t, H * 64, "attn_decode_out", "q/k/v/o");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "aiko.attn_decode_out: 16-byte alignment");
  }
  TORCH_CHECK(q.size(0) == B && o.size(0) == B, "aiko.attn_decode_out: q/o need B rows");
  TORCH_CHECK(k.size(0) == B * S && v.size(0) == B * S, "aiko.attn_decode_out: k/v need B*S rows");
  const void *kn = nullptr, *vn = nullptr;
  int64_t ldnew = 0;
  const int* pp = nullptr;
  if (app) {
    check_i32(*pos, 1, "pos");
    pp = pos->data_ptr<int>();
    TORCH_CHECK(knew.has_value() && knew->defined() && vnew.has_value() && vnew->defined(),
                "aiko.attn_decode_out: append mode needs knew and vnew");
    for (const at::Tensor* t : {&*knew, &*vnew}) {
      check_cuda(*t, "knew/vnew");
      TORCH_CHECK(t->scalar_type() == at::kBFloat16 && t->size(0) == B &&
                      reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                  "aiko.attn_decode_out: knew/vnew bf16 [B, >= H*64], 16-byte aligned");
      row_pitch(*t, H * 64, "attn_decode_out", "knew/vnew");
    }
    TORCH_CHECK(knew->stride(0) == vnew->stride(0), "aiko.attn_decode_out: knew/vnew must share a row pitch");
    kn = knew->data_ptr();
    vn = vnew->data_ptr();
    ldnew = knew->stride(0);
  } else {
    TORCH_CHECK(T >= 1 && T <= S, "aiko.attn_decode_out: 1 <= T <= S");
  }
  check_cuda(work, "work");
  TORCH_CHECK(work.scalar_type() == at::kFloat && work.is_contiguous(), "aiko.attn_decode_out: work fp32");
  TORCH_CHECK(work.numel() >= aiko_attn_decode_work(B, H, app ? S : T), "aiko.attn_decode_out: work too small");
  check_launch(aiko_attn_decode(q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0), v.stride(0), S, pp,
                                T, kn, vn, ldnew, o.data_ptr(), o.stride(0), B, H, (float)scale,
                                work.data_ptr<float>(), work.numel(), cur_stream()),
               "attn_decode");
}


// y = act(LN?(x) quantised per row to e4m3 @ W^T * scales + bias) (+ res): the decoder's fused
// skinny-M linear (x bf16 [M, K], K % 128 == 0, K <= 3072; W e4m3 [N, K])
void dec_linear_out(const at::Tensor& x, const c10::optional<at::Tensor>& gamma, const c10::optional<at::Tensor>& beta,
                    double eps, const at::Tensor& w, const at::Tensor& sw, const c10::optional<at::Tensor>& bias,
                    const c10::optional<at::Tensor>& res, at::Tensor& y, int64_t act) {
  for (const at::Tensor* t : {&x, &w, &sw, (const at::Tensor*)&y}) check_cuda(*t, "dec_linear operand");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && y.scalar_type() == at::kBFloat16, "aiko.dec_linear_out: bf16 x / y");
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.element_size() == 1 && w.dim() == 2 && w.size(1) == K && w.is_contiguous(),
              "aiko.dec_linear_out: w e4m3 [N, K] contiguous with K == x width");
  TORCH_CHECK(K % 128 == 0 && K <= 3072, "aiko.dec_linear_out: K % 128 == 0 and K <= 3072");
  TORCH_CHECK(sw.scalar_type() == at::kFloat && sw.numel() == N && sw.is_contiguous(), "aiko.dec_linear_out: sw fp32 [N]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "aiko.dec_linear_out: x / w 16-byte alignment");
  const int64_t ldx = row_pitch(x, K, "dec_linear_out", "x");
  TORCH_CHECK(y.size(0) == M, "aiko.dec_linear_out: y [M, N]");
  const int64_t ldy = row_pitch(y, N, "dec_linear_out", "y");
  const float *g = nullptr, *be = nullptr, *bp = nullptr;
  if (gamma.has_value() && gamma->defined()) {
    TORCH_CHECK(beta.has_value() && beta->defined(), "aiko.dec_linear_out: gamma needs beta");
    for (const at::Tensor* t : {&*gamma, &*beta}) {
      check_cuda(*t, "gamma/beta");
      TORCH_CHECK(t->scalar_type() == at::kFloat && t->numel() == K && t->is_contiguous(), "aiko.dec_linear_out: gamma/beta fp32 [K]");
    }
    g = gamma->data_ptr<float>();
    be = beta->data_ptr<float>();
  }
  if (bias.has_value() && bias->defined()) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == N && bias->is_contiguous(), "aiko.dec_linear_out: bias fp32 [N]");
    bp = bias->data_ptr<float>();
  }
  const void* rp = nullptr;
  int64_t ldr = 0;
  if (res.has_value() && res->defined()) {
    check_cuda(*res, "residual");
    TORCH_CHECK(res->scalar_type() == at::kBFloat16 && res->size(0) == M, "aiko.dec_linear_out: residual bf16 [M, N]");
    ldr = row_pitch(*res, N, "dec_linear_out", "residual");
    rp = res->data_ptr();
  }
  check_launch(aiko_dec_linear(x.data_ptr(), ldx, g, be, (float)eps, w.data_ptr(), sw.data_ptr<float>(), bp, rp, ldr,
                               y.data_ptr(), ldy, M, N, K, act, cur_stream()),
               "dec_linear");
}

// greedy next token per sequence; advances pos[0] on the device (see decode_ops.hip)
void argmax_step_out(const at::Tensor& logits, int64_t V, at::Tensor& ids, at::Tensor& pos, at::Tensor& out_tokens,
                     const at::Tensor& forced, int64_t eot, at::Tensor& done, at::Tensor& counter) {
  check_cuda(logits, "logits");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 && logits.dim() == 2 && logits.stride(1) == 1 &&
                  reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0,
              "aiko.argmax_step_out: logits bf16 [B, >= V], 16-byte aligned rows");
  const int64_t B = logits.size(0);
  check_i32(ids, B, "ids");
  check_i32(pos, 1, "pos");
  check_i32(done, B, "done");
  check_i32(counter, 1, "counter");
  check_cuda(out_tokens, "out_tokens");
  TORCH_CHECK(out_tokens.scalar_type() == at::kInt && out_tokens.dim() == 2 && out_tokens.size(0) == B &&
                  out_tokens.is_contiguous(),
              "aiko.argmax_step_out: out_tokens int32 [B, max_len]");
  check_i32(forced, 1, "forced");
  check_launch(aiko_argmax_step(logits.data_ptr(), logits.stride(0), V, B, ids.data_ptr<int>(), pos.data_ptr<int>(),
                                out_tokens.data_ptr<int>(), out_tokens.size(1), forced.data_ptr<int>(), forced.numel(),
                                eot, done.data_ptr<int>(), reinterpret_cast<unsigned*>(counter.data_ptr<int>()),
                                cur_stream()),
               "argmax_step");
}

}  // namespace

TORCH_LIBRARY(aiko, m) {
  m.def("conv_igemm_out(Tensor x, Tensor? x2, Tensor w, Tensor? bias, Tensor? res, Tensor(a!) y, int[] geom, Tensor? zero=None) -> ()");
  m.def("preprocess_out(Tensor frames, Tensor(a!) out, int Ho, int Wo, int pad_t, int pad_l, float[] mean, float[] std, bool bgr, float[] canvas=[]) -> ()");
  m.def("upsample2x_out(Tensor x, Tensor(a!) y) -> ()");
  m.def("resize_u8_out(Tensor x, Tensor(a!) y) -> ()");
  m.def("roi_crop_out(Tensor frames, Tensor det, Tensor count, int k, float margin, Tensor(a!) crops, Tensor(b!) rois) -> ()");
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

TORCH_LIBRARY_IMPL(aiko, CUDA, m) {
  m.impl("conv_igemm_out", &conv_igemm_out);
  m.impl("preprocess_out", &preprocess_out);
  m.impl("maxpool_out", &maxpool_out);
  m.impl("conv_chain_out", &conv_chain_out);
  m.impl("bneck_fused_out", &bneck_fused_out);
  m.impl("conv3x3_exp_out", &conv3x3_exp_out);
  m.impl("conv3x3_patch_out", &conv3x3_patch_out);
  m.impl("conv3x3_patchw_out", &conv3x3_patchw_out);
  m.impl("conv3x3_rows_out", &conv3x3_rows_out);
  m.impl("stem_direct_out", &stem_direct_out);
  m.impl("upsample2x_out", &upsample2x_out);
  m.impl("resize_u8_out", &resize_u8_out);
  m.impl("roi_crop_out", &roi_crop_out);
  m.impl("draw_detections_out", &draw_detections_out);
  m.impl("redact_detections_out", &redact_detections_out);
  m.impl("yuv_to_rgb_out", &yuv_to_rgb_out);
  m.impl("rgb_to_yuv_out", &rgb_to_yuv_out);
  m.impl("batchnorm_out", &batchnorm_out);
  m.impl("yolo_decode_out", &yolo_decode_out);
  m.impl("topk_nms_out", &topk_nms_out);
  m.impl("avgpool_out", &avgpool_out);
  m.impl("mean_rows_out", &mean_rows_out);
  m.impl("window_shift_out", &window_shift_out);
  m.impl("resample_out", &resample_out);
  m.impl("track_detections_out", &track_detections_out);
  m.impl("marker_detect_out", &marker_detect_out);
  m.impl("motion_detect_out", &motion_detect_out);
  m.impl("voice_activity_out", &voice_activity_out);
  m.impl("spectrum_out", &spectrum_out);
  m.impl("spectrum_graph_out", &spectrum_graph_out);
  m.impl("jpeg_encode_out", &jpeg_encode_out);
  m.impl("jpeg_decode_out", &jpeg_decode_out);
  m.impl("zero_border_rows_", &zero_border_rows_);
  m.impl("sppf_pool_", &sppf_pool_);
  m.impl("stem_pool_out", &stem_pool_out);
  m.impl("stem_pool_u8_out", &stem_pool_u8_out);
  m.impl("softmax_topk_out", &softmax_topk_out);
  m.impl("gemm_fp8_out", &gemm_fp8_out);
  m.impl("rownorm_quant_out", &rownorm_quant_out);
  m.impl("c2f_fused_out", &c2f_fused_out);
  m.impl("c2f_bneck_out", &c2f_bneck_out);
  m.impl("conv_glds_tail_out", &conv_glds_tail_out);
  m.impl("conv_glds_tail_decode_out", &conv_glds_tail_decode_out);
  m.impl("attn_fwd_out", &attn_fwd_out);
  m.impl("linear_splitk_out", &linear_splitk_out);
  m.impl("logmel_out", &logmel_out);
  m.impl("embed_tokens_out", &embed_tokens_out);
  m.impl("attn_decode_out", &attn_decode_out);
  m.impl("argmax_step_out", &argmax_step_out);
  m.impl("dec_linear_out", &dec_linear_out);
}
