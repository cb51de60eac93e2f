// What every binding file shares: the torch / HIP headers, the launchers' declarations
// (kernels/aiko_api.h) and the argument checks that several operators repeat.  The checks fail
// loudly (TORCH_CHECK) with the operator's name in front; none launches or allocates anything.
// Everything here is inline in an unnamed namespace: each binding file has its own copy.
#pragma once

#include <ATen/core/Tensor.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <vector>

#include "kernels/aiko_api.h"

namespace {

using TensorPtrs = at::ArrayRef<const at::Tensor*>;
using Names = at::ArrayRef<const char*>;

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline void check_cuda(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "aiko: ", name, " must be a GPU tensor");
}

// elements addressable from t.data_ptr() to the end of its storage
inline int64_t avail_elems(const at::Tensor& t) {
  return (int64_t)(t.storage().nbytes() / t.element_size()) - t.storage_offset();
}

inline void check_launch(int rc, const char* what) {
  TORCH_CHECK(rc == 0, "aiko: launch of ", what, " failed: ",
              rc < 0 ? "unsupported configuration" : hipGetErrorString((hipError_t)rc));
}

inline void check_i32(const at::Tensor& t, int64_t n, const char* what) {
  check_cuda(t, what);
  TORCH_CHECK(t.scalar_type() == at::kInt && t.is_contiguous() && t.numel() >= n, "aiko: ", what,
              " must be contiguous int32 with >= ", n, " elements");
}

// an optional tensor that was passed and is not None
inline bool defined(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); }

inline bool aligned(const at::Tensor& t, uintptr_t bytes) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0;
}

// NHWC bf16 tensor whose channels may be a slice of a wider buffer: returns the pixel pitch
inline int64_t pixel_pitch(const at::Tensor& t, const char* op) {
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.dim() == 4, "aiko.", op, ": NHWC bf16 tensors required");
  const int64_t C = t.size(3), ld = t.stride(2);
  TORCH_CHECK(t.stride(3) == 1 && t.stride(1) == t.size(2) * ld && t.stride(0) == t.size(1) * t.stride(1) &&
                  ld % 8 == 0 && C % 8 == 0 && aligned(t, 16),
              "aiko.", op, ": tensor must be NHWC with unit channel stride, C and pitch multiples of 8");
  TORCH_CHECK(avail_elems(t) >= (t.size(0) * t.size(1) * t.size(2) - 1) * ld + C, "aiko.", op, ": storage too small");
  return ld;
}

// what every frames argument has in common; an operator's own extras (a numel() floor) stay with it
inline void check_frames_u8(const at::Tensor& t, const char* op) {
  TORCH_CHECK(t.scalar_type() == at::kByte && t.dim() == 4 && t.size(3) == 3 && t.is_contiguous(),
              "aiko.", op, ": frames uint8 [B, H, W, 3] contiguous required");
}

// detector rows [B, max_det, 6]: returns max_det
inline int64_t check_det(const at::Tensor& det, int64_t B, const char* op) {
  TORCH_CHECK(det.scalar_type() == at::kFloat && det.dim() == 3 && det.size(0) == B && det.size(2) == 6 &&
                  det.is_contiguous(),
              "aiko.", op, ": det fp32 [B, max_det, 6] contiguous required");
  return det.size(1);
}

// a detector's output as an operator's input: det [B, max_det, 6] and count [B]; returns max_det
inline int64_t check_det_count(const at::Tensor& det, const at::Tensor& count, int64_t B, const char* op) {
  const int64_t max_det = check_det(det, B, op);
  TORCH_CHECK(count.scalar_type() == at::kInt && count.dim() == 1 && count.size(0) == B && count.is_contiguous(),
              "aiko.", op, ": count int32 [B] contiguous required");
  return max_det;
}

inline void check_k(int64_t k, int64_t max_det, const char* op) {
  TORCH_CHECK(k >= 1 && k <= max_det, "aiko.", op, ": 1 <= k <= max_det (", max_det, ") required, got ", k);
}

inline void check_cuda_all(TensorPtrs ts, Names names) {
  for (size_t i = 0; i < ts.size(); ++i) check_cuda(*ts[i], names[i]);
}

// every tensor is on the first one's device
inline void check_same_device(TensorPtrs ins, TensorPtrs outs, const char* op) {
  for (const TensorPtrs& ts : {ins, outs})
    for (const at::Tensor* t : ts)
      TORCH_CHECK(t->device() == ins[0]->device(), "aiko.", op, ": tensors on different devices");
}

inline bool overlap(const at::Tensor& x, const at::Tensor& y) {
  const auto xp = reinterpret_cast<uintptr_t>(x.data_ptr()), yp = reinterpret_cast<uintptr_t>(y.data_ptr());
  const uintptr_t xn = x.numel() * x.element_size(), yn = y.numel() * y.element_size();
  return xn > 0 && yn > 0 && xp < yp + yn && yp < xp + xn;
}

// no output may overlap an input or an earlier output (contiguous tensors)
inline void check_no_overlap(TensorPtrs outs, Names out_names, TensorPtrs ins, Names in_names, const char* op) {
  for (size_t o = 0; o < outs.size(); ++o) {
    for (size_t i = 0; i < ins.size(); ++i)
      TORCH_CHECK(!overlap(*outs[o], *ins[i]), "aiko.", op, ": ", out_names[o], " and ", in_names[i], " overlap");
    for (size_t p = 0; p < o; ++p)
      TORCH_CHECK(!overlap(*outs[o], *outs[p]), "aiko.", op, ": ", out_names[o], " and ", out_names[p], " overlap");
  }
}

// out is frames itself (in place) or does not touch it; both uint8 of one shape
inline void check_inplace_or_disjoint(const at::Tensor& frames, const at::Tensor& out, const char* op) {
  const auto fp = reinterpret_cast<uintptr_t>(frames.data_ptr()), op_ = reinterpret_cast<uintptr_t>(out.data_ptr());
  const uintptr_t nbytes = (uintptr_t)frames.numel();
  TORCH_CHECK(fp == op_ || fp + nbytes <= op_ || op_ + nbytes <= fp,
              "aiko.", op, ": out overlaps frames without being the same tensor");
}

// the launch grid of the kernels that walk a frame in tiles of 32 rows: (tile rows, frames)
inline void check_tile_grid(int64_t B, int64_t H, int64_t W, const char* op) {
  TORCH_CHECK(B <= 65535 && (H + 31) / 32 <= 65535 && H <= (1 << 24) && W <= (1 << 24),
              "aiko.", op, ": B = ", B, ", H = ", H, ", W = ", W,
              " exceed the grid limit (65535 frames, 65535 tile rows of 32, side <= 2^24)");
}

// N coefficients (``names`` lists them for the message), each finite as an fp32 value
template <int N>
inline void to_finite_floats(at::ArrayRef<double> coeffs, float (&out)[N], const char* op, const char* names) {
  TORCH_CHECK(coeffs.size() == N, "aiko.", op, ": ", N, " coefficients (", names, ") required, got ", coeffs.size());
  for (int i = 0; i < N; ++i) {
    out[i] = (float)coeffs[i];
    TORCH_CHECK(std::isfinite(out[i]), "aiko.", op, ": coefficient ", i, " is not finite in fp32");
  }
}

}  // namespace
