// torch.ops.aiko.*: raw YUV frames and JPEG streams in and out.
// Each operator validates shapes / dtypes / devices on the host (checks.h holds the shared
// checks) and launches on the caller's current HIP stream.
#include "checks.h"

namespace {

// out [B, H, W, 3] <- raw [B, frame_bytes] YUV frames, tightly packed.  format: 0 nv12, 1 i420,
// 2 i444, 3 yuyv; coeffs: yoff, ygain, rv, gu, gv, bu; round_mode: 0 rint, 1 add half and truncate
void yuv_to_rgb_out(const at::Tensor& raw, int64_t height, int64_t width, int64_t format,
                    at::ArrayRef<double> coeffs, int64_t round_mode, at::Tensor& out) {
  check_cuda(raw, "raw");
  check_cuda(out, "out");
  TORCH_CHECK(raw.device() == out.device(), "aiko.yuv_to_rgb_out: raw and out on different devices");
  TORCH_CHECK(format >= 0 && format <= 3, "aiko.yuv_to_rgb_out: unknown format code ", format);
  TORCH_CHECK(round_mode == 0 || round_mode == 1, "aiko.yuv_to_rgb_out: unknown round mode ", round_mode);
  float coef[6];
  to_finite_floats(coeffs, coef, "yuv_to_rgb_out", "yoff, ygain, rv, gu, gv, bu");
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
  float coef[10];
  to_finite_floats(coeffs, coef, "rgb_to_yuv_out", "yoff, yr, yg, yb, ur, ug, ub, vr, vg, vb");
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

// Baseline JPEG (jpeg_ops.hip; the rule is in ops/jpeg.py): raw planar frames [B, frame_bytes] (fmt 1: i420,
// 2: i444) -> one JFIF stream per frame in stream [B, cap], its length (-1: overflow) in nbytes [B].  tables is
// ops.jpeg.device_tables' tensor (864 words, then header_len bytes of header); workspace holds an int32 and
// seg_cap bytes per (frame, MCU row).  Two launches on the current stream
void jpeg_encode_out(const at::Tensor& raw, int64_t height, int64_t width, int64_t fmt, const at::Tensor& tables,
                     int64_t header_len, int64_t seg_cap, at::Tensor& stream, at::Tensor& nbytes,
                     at::Tensor& workspace) {
  const at::Tensor* ins[2] = {&raw, &tables};
  const char* in_names[2] = {"raw", "tables"};
  const at::Tensor* outs[3] = {&stream, &nbytes, &workspace};
  const char* out_names[3] = {"stream", "nbytes", "workspace"};
  check_cuda_all(ins, in_names);
  check_cuda_all(outs, out_names);
  check_same_device(ins, outs, "jpeg_encode_out");
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
                  tables.numel() == 4 * 864 + header_len && aligned(tables, 4),
              "aiko.jpeg_encode_out: tables uint8 [3456 + header_len] contiguous, 4-byte aligned required");
  TORCH_CHECK(stream.scalar_type() == at::kByte && stream.dim() == 2 && stream.size(0) == B && stream.size(1) >= 1 &&
                  stream.size(1) <= INT_MAX && stream.is_contiguous(),
              "aiko.jpeg_encode_out: stream uint8 [B, cap] contiguous required, 1 <= cap < 2^31");
  TORCH_CHECK(nbytes.scalar_type() == at::kInt && nbytes.dim() == 1 && nbytes.size(0) == B && nbytes.is_contiguous(),
              "aiko.jpeg_encode_out: nbytes int32 [B] contiguous required");
  const int64_t need = B * my * (4 + seg_cap);
  TORCH_CHECK(workspace.scalar_type() == at::kByte && workspace.dim() == 1 && workspace.is_contiguous() &&
                  workspace.numel() >= need && aligned(workspace, 4),
              "aiko.jpeg_encode_out: workspace uint8 [>= ", need, "] contiguous, 4-byte aligned required");
  // no output may overlap an input or another output
  check_no_overlap(outs, out_names, ins, in_names, "jpeg_encode_out");
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
  const at::Tensor* ins[3] = {&data, &nbytes, &desc};
  const char* in_names[3] = {"data", "nbytes", "desc"};
  const at::Tensor* outs[3] = {&raw, &status, &workspace};
  const char* out_names[3] = {"raw", "status", "workspace"};
  check_cuda_all(ins, in_names);
  check_cuda_all(outs, out_names);
  check_same_device(ins, outs, "jpeg_decode_out");
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
                  desc.size(1) == 1744 && desc.is_contiguous() && aligned(desc, 4),
              "aiko.jpeg_decode_out: desc uint8 [B, 1744] or [1, 1744] contiguous, 4-byte aligned required");
  TORCH_CHECK(raw.scalar_type() == at::kByte && raw.dim() == 2 && raw.size(0) == B && raw.size(1) == frame &&
                  raw.is_contiguous(),
              "aiko.jpeg_decode_out: raw uint8 [B, ", frame, "] contiguous required");
  TORCH_CHECK(status.scalar_type() == at::kInt && status.dim() == 1 && status.size(0) == B && status.is_contiguous(),
              "aiko.jpeg_decode_out: status int32 [B] contiguous required");
  const int64_t need = (4 * B * (1 + 2 * max_intervals) + 15) / 16 * 16 + B * nblocks * 128;
  TORCH_CHECK(workspace.scalar_type() == at::kByte && workspace.dim() == 1 && workspace.is_contiguous() &&
                  workspace.numel() >= need && aligned(workspace, 16),
              "aiko.jpeg_decode_out: workspace uint8 [>= ", need, "] contiguous, 16-byte aligned required");
  // no output may overlap an input or another output
  check_no_overlap(outs, out_names, ins, in_names, "jpeg_decode_out");
  check_launch(aiko_jpeg_decode(data.data_ptr(), nbytes.data_ptr<int>(), desc.data_ptr(), (int)desc.size(0),
                                workspace.data_ptr(), raw.data_ptr(), status.data_ptr<int>(), (int)B, (int)H, (int)W,
                                (int)fmt, (long)data.size(1), (int)max_intervals, cur_stream()),
               "jpeg_decode");
}

}  // namespace

TORCH_LIBRARY_IMPL(aiko, CUDA, m) {
  m.impl("yuv_to_rgb_out", &yuv_to_rgb_out);
  m.impl("rgb_to_yuv_out", &rgb_to_yuv_out);
  m.impl("jpeg_encode_out", &jpeg_encode_out);
  m.impl("jpeg_decode_out", &jpeg_decode_out);
}
