// torch.ops.aiko.*: pre-processing, pools, normalisation and the classifier's tail.
// Each operator validates shapes / dtypes / devices on the host (checks.h holds the shared
// checks) and launches on the caller's current HIP stream.
#include "checks.h"

namespace {

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

// One axis of a scale plan (ops/scale.py): bounds int32 [n_out, 2] and coefficients int32
// [n_out, ksize], both given or both left out (then the axis keeps its size).  Returns ksize, or 0
// without the pass.  What the tables hold (first + n <= in_size per entry) is checked on the host
// when the plan is made; here they lie in HBM, and the kernel clamps what it reads from them.
int64_t check_scale_axis(const at::Tensor& frames, const c10::optional<at::Tensor>& bounds,
                         const c10::optional<at::Tensor>& coeffs, int64_t n_in, int64_t n_out, const char* axis) {
  TORCH_CHECK(defined(bounds) == defined(coeffs), "aiko.scale_frames_out: the ", axis,
              " bounds and coefficients are given together or not at all");
  if (!defined(bounds)) {
    TORCH_CHECK(n_out == n_in, "aiko.scale_frames_out: without a ", axis, " plan out keeps that size, ", n_in,
                ", got ", n_out);
    return 0;
  }
  check_cuda_all({&*bounds, &*coeffs}, {"bounds", "coefficients"});
  check_same_device({&frames}, {&*bounds, &*coeffs}, "scale_frames_out");
  TORCH_CHECK(bounds->scalar_type() == at::kInt && bounds->dim() == 2 && bounds->size(0) == n_out &&
                  bounds->size(1) == 2 && bounds->is_contiguous() && aligned(*bounds, 8),
              "aiko.scale_frames_out: ", axis, " bounds int32 [", n_out, ", 2] contiguous, 8-byte aligned required");
  TORCH_CHECK(coeffs->scalar_type() == at::kInt && coeffs->dim() == 2 && coeffs->size(0) == n_out &&
                  coeffs->size(1) >= 1 && coeffs->size(1) <= INT_MAX && coeffs->is_contiguous(),
              "aiko.scale_frames_out: ", axis, " coefficients int32 [", n_out, ", ksize >= 1] contiguous required");
  return coeffs->size(1);
}

// The antialiased resize (scale_ops.hip; the rule is in ops/scale.py): frames [B, H, W, 3] -> out
// [B, Ho, Wo, 3] by the horizontal plan (hb, hk) and the vertical plan (vb, vk).  With both, a
// workgroup makes tile_rows x tile_cols output pixels from at most win_rows source rows.
void scale_frames_out(const at::Tensor& frames, const c10::optional<at::Tensor>& hb,
                      const c10::optional<at::Tensor>& hk, const c10::optional<at::Tensor>& vb,
                      const c10::optional<at::Tensor>& vk, int64_t tile_rows, int64_t tile_cols, int64_t win_rows,
                      at::Tensor& out) {
  check_cuda_all({&frames, &out}, {"frames", "out"});
  check_same_device({&frames}, {&out}, "scale_frames_out");
  check_frames_u8(frames, "scale_frames_out");
  const int64_t B = frames.size(0), H = frames.size(1), W = frames.size(2);
  const int64_t side = 1 << 24;
  TORCH_CHECK(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= side && W <= side,
              "aiko.scale_frames_out: 1..65535 frames with sides 1..2^24 required, got ", B, " x ", H, " x ", W);
  TORCH_CHECK(out.scalar_type() == at::kByte && out.dim() == 4 && out.size(0) == B && out.size(1) >= 1 &&
                  out.size(2) >= 1 && out.size(1) <= side && out.size(2) <= side && out.size(3) == 3 &&
                  out.is_contiguous(),
              "aiko.scale_frames_out: out uint8 [", B, ", Ho, Wo, 3] contiguous with sides 1..2^24 required");
  const int64_t Ho = out.size(1), Wo = out.size(2);
  const int64_t ksh = check_scale_axis(frames, hb, hk, W, Wo, "horizontal");
  const int64_t ksv = check_scale_axis(frames, vb, vk, H, Ho, "vertical");
  TORCH_CHECK(ksh > 0 || ksv > 0, "aiko.scale_frames_out: no pass to run (out has the frames' size): copy instead");
  if (ksh > 0 && ksv > 0) {
    TORCH_CHECK(tile_rows >= 1 && tile_rows <= Ho && tile_cols >= 4 && tile_cols <= 64 && tile_cols % 4 == 0,
                "aiko.scale_frames_out: a tile of 1..Ho rows and 4..64 columns, a multiple of 4, required, got ",
                tile_rows, " x ", tile_cols);
    TORCH_CHECK(win_rows >= 1 && win_rows <= H && win_rows * tile_cols * 3 <= 160 * 1024,
                "aiko.scale_frames_out: a window of 1..H rows that fits 160 KiB of LDS required, got ", win_rows,
                " rows x ", tile_cols, " columns");
  }
  std::vector<const at::Tensor*> ins = {&frames};
  std::vector<const char*> in_names = {"frames"};
  if (ksh > 0) {
    ins.insert(ins.end(), {&*hb, &*hk});
    in_names.insert(in_names.end(), {"the horizontal bounds", "the horizontal coefficients"});
  }
  if (ksv > 0) {
    ins.insert(ins.end(), {&*vb, &*vk});
    in_names.insert(in_names.end(), {"the vertical bounds", "the vertical coefficients"});
  }
  check_no_overlap({&out}, {"out"}, ins, in_names, "scale_frames_out");
  check_launch(aiko_scale_frames(frames.data_ptr(), ksh ? hb->data_ptr<int>() : nullptr,
                                 ksh ? hk->data_ptr<int>() : nullptr, ksv ? vb->data_ptr<int>() : nullptr,
                                 ksv ? vk->data_ptr<int>() : nullptr, out.data_ptr(), (int)B, (int)H, (int)W, (int)Ho,
                                 (int)Wo, (int)ksh, (int)ksv, (int)tile_rows, (int)tile_cols, (int)win_rows,
                                 cur_stream()),
               "scale_frames");
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
  TORCH_CHECK(aligned(x, 16) && x.stride(0) % 8 == 0,
              "aiko.mean_rows_out: 16-byte aligned rows");
  TORCH_CHECK(avail_elems(x) >= (B - 1) * x.stride(0) + T * C, "aiko.mean_rows_out: x storage too small");
  check_launch(aiko_mean_rows_f32(x.data_ptr(), y.data_ptr<float>(), B, T, C, (long)x.stride(0), cur_stream()),
               "mean_rows");
}

void batchnorm_out(const at::Tensor& x, const at::Tensor& scale, const at::Tensor& shift, at::Tensor& y, int64_t act) {
  check_cuda_all({&x, &y, &scale, &shift}, {"x", "y", "scale", "shift"});
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
  TORCH_CHECK(aligned(x, 16), "aiko.zero_border_rows_: alignment");
  check_launch(aiko_zero_border_rows(x.data_ptr(), x.size(0) / rows, rows, x.size(1), cur_stream()),
               "zero_border_rows");
}

void softmax_topk_out(const at::Tensor& logits, at::Tensor& prob, at::Tensor& index, int64_t k) {
  check_cuda_all({&logits, &prob, &index}, {"logits", "prob", "index"});
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

void window_shift_out(const at::Tensor& src, const at::Tensor& chunk, at::Tensor& dst) {
  check_cuda_all({&src, &chunk, &dst}, {"src", "chunk", "dst"});
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

}  // namespace

TORCH_LIBRARY_IMPL(aiko, CUDA, m) {
  m.impl("preprocess_out", &preprocess_out);
  m.impl("resize_u8_out", &resize_u8_out);
  m.impl("scale_frames_out", &scale_frames_out);
  m.impl("maxpool_out", &maxpool_out);
  m.impl("avgpool_out", &avgpool_out);
  m.impl("mean_rows_out", &mean_rows_out);
  m.impl("batchnorm_out", &batchnorm_out);
  m.impl("upsample2x_out", &upsample2x_out);
  m.impl("sppf_pool_", &sppf_pool_);
  m.impl("zero_border_rows_", &zero_border_rows_);
  m.impl("softmax_topk_out", &softmax_topk_out);
  m.impl("window_shift_out", &window_shift_out);
}
