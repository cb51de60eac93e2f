// torch.ops.aiko.*: convolutions: the implicit-GEMM dispatch, the LDS-resident 3x3 kernels, the fused blocks and the stems.
// Each operator validates shapes / dtypes / devices on the host (checks.h holds the shared
// checks) and launches on the caller's current HIP stream.
#include "checks.h"

namespace {

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
  check_cuda_all({&x, &w, &y}, {"x", "w", "y"});
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16 &&
                  y.scalar_type() == at::kBFloat16,
              "aiko.conv_igemm_out: x, w, y must be bfloat16");
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous(), "aiko.conv_igemm_out: w must be [Cout, K] contiguous");
  const int64_t Cout = w.size(0), K = w.size(1);
  const bool dual = defined(x2);
  const int64_t Kmain = dual ? K1 : K;
  TORCH_CHECK(Kmain >= R * S * Cc && Kmain % 64 == 0 && Kmain - R * S * Cc < 64, "aiko.conv_igemm_out: K=",
              Kmain, " must be R*S*Cc rounded up to a multiple of 64");
  const void* x2ptr = nullptr;
  if (dual) {
    check_cuda(*x2, "x2");
    TORCH_CHECK(x2->scalar_type() == at::kBFloat16, "aiko.conv_igemm_out: x2 must be bf16");
    TORCH_CHECK((K - K1) % 64 == 0 && K - K1 <= C2 && C2 % 8 == 0 && K1 > 0,
                "aiko.conv_igemm_out: second source needs K-K1 (multiple of 64) <= C2");
    TORCH_CHECK(aligned(*x2, 16), "aiko.conv_igemm_out: x2 alignment");
    TORCH_CHECK(M % (Ho * Wo) == 0 && (Ho - 1) * stride2 < H2 && (Wo - 1) * stride2 < W2 &&
                    avail_elems(*x2) >= (M / (Ho * Wo)) * H2 * W2 * C2,
                "aiko.conv_igemm_out: x2 too small for the output geometry");
    x2ptr = x2->data_ptr();
  }
  TORCH_CHECK(Cc % 8 == 0 && (Cc <= C || C == 4), "aiko.conv_igemm_out: Cc must be a multiple of 8 within the pixel pitch (or span pixels of a 4-channel stem input)");
  TORCH_CHECK(Cout % 8 == 0, "aiko.conv_igemm_out: Cout must be a multiple of 8");
  TORCH_CHECK(C % 8 == 0 || (C == 4 && Cc % 8 == 0), "aiko.conv_igemm_out: pixel pitch must keep 16-B alignment");
  TORCH_CHECK(aligned(x, 16) && aligned(y, 16), "aiko.conv_igemm_out: x and y must be 16-byte aligned");
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
  if (defined(bias)) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == Cout && bias->is_contiguous(),
                "aiko.conv_igemm_out: bias must be fp32 [Cout]");
    bptr = bias->data_ptr<float>();
  }
  const void* rptr = nullptr;
  if (defined(res)) {
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
      TORCH_CHECK(defined(zero) && zero->is_cuda() && zero->nbytes() >= 16 &&
                      aligned(*zero, 16),
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

// 3x3 / stride 1 / pad 1 conv, 64 -> 64 channels, with an LDS-resident input patch (conv_patch.hip).
// x [B, H, W, 64] contiguous; wimg the [9, 2, 4, 64, 8] fragment image (ops.conv.patch_weight);
// y [B, H, W, >= 64] NHWC with unit channel stride (a channel slice of a wider buffer is fine).
void conv3x3_patch_out(const at::Tensor& x, const at::Tensor& wimg, const c10::optional<at::Tensor>& bias,
                       at::Tensor& y, int64_t act, int64_t grid) {
  check_cuda_all({&x, &wimg, &y}, {"x", "wimg", "y"});
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && wimg.scalar_type() == at::kBFloat16 && y.scalar_type() == at::kBFloat16,
              "aiko.conv3x3_patch_out: bf16 tensors");
  TORCH_CHECK(x.dim() == 4 && x.size(3) == 64 && x.is_contiguous(), "aiko.conv3x3_patch_out: x must be [B, H, W, 64] contiguous");
  TORCH_CHECK(wimg.is_contiguous() && wimg.numel() == 9 * 64 * 64, "aiko.conv3x3_patch_out: wimg must be the 36864-element image");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2);
  TORCH_CHECK(W + 8 <= 64, "aiko.conv3x3_patch_out: W <= 56");
  TORCH_CHECK(y.dim() == 4 && y.size(0) == B && y.size(1) == H && y.size(2) == W && y.size(3) == 64 && y.stride(3) == 1 &&
                  y.stride(2) % 8 == 0 && y.stride(1) == W * y.stride(2) && y.stride(0) == H * W * y.stride(2) &&
                  aligned(y, 16),
              "aiko.conv3x3_patch_out: y must be [B, H, W, 64] NHWC (16-B aligned pixel pitch)");
  TORCH_CHECK(x.numel() * 2 < (1LL << 31) - 64 && avail_elems(y) * 2 < (1LL << 31) - 64,
              "aiko.conv3x3_patch_out: tensors too large for 32-bit offsets");
  TORCH_CHECK(act == 0 || act == 1 || act == 2, "aiko.conv3x3_patch_out: act none / relu / silu");
  const float* bptr = nullptr;
  if (defined(bias)) {
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
  check_cuda_all({&x, &wimg, &y}, {"x", "wimg", "y"});
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && wimg.scalar_type() == at::kBFloat16 && y.scalar_type() == at::kBFloat16,
              "aiko.conv3x3_patchw_out: bf16 tensors");
  TORCH_CHECK(x.dim() == 4 && x.size(3) >= 128 && x.size(2) == 28 && x.stride(3) == 1 && x.stride(2) % 8 == 0 &&
                  x.stride(1) == 28 * x.stride(2) && x.stride(0) == x.size(1) * x.stride(1) &&
                  aligned(x, 16),
              "aiko.conv3x3_patchw_out: x must be [B, H, 28, >= 128] NHWC with a 16-B aligned pixel pitch");
  TORCH_CHECK(wimg.is_contiguous() && wimg.numel() == 9 * 128 * 128, "aiko.conv3x3_patchw_out: wimg must be the 147456-element image");
  const int64_t B = x.size(0), H = x.size(1), W = x.size(2);
  TORCH_CHECK(y.dim() == 4 && y.size(0) == B && y.size(1) == H && y.size(2) == W && y.size(3) == 128 && y.stride(3) == 1 &&
                  y.stride(2) % 8 == 0 && y.stride(1) == W * y.stride(2) && y.stride(0) == H * W * y.stride(2) &&
                  aligned(y, 16),
              "aiko.conv3x3_patchw_out: y must be [B, H, 28, 128] NHWC (16-B aligned pixel pitch)");
  TORCH_CHECK(avail_elems(x) * 2 < (1LL << 31) - 64 && avail_elems(y) * 2 < (1LL << 31) - 64,
              "aiko.conv3x3_patchw_out: tensors too large for 32-bit offsets");
  TORCH_CHECK(act == 0 || act == 1, "aiko.conv3x3_patchw_out: act none / relu");
  const float* bptr = nullptr;
  if (defined(bias)) {
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
  check_cuda_all({&x, &wimg, &y}, {"x", "wimg", "y"});
  auto rows_ok = [](const at::Tensor& t, int64_t B, int64_t H) {
    return t.dim() == 4 && t.size(0) == B && t.size(1) == H && t.size(2) == 80 && t.size(3) >= 32 && t.stride(3) == 1 &&
           t.stride(2) % 8 == 0 && t.stride(1) == 80 * t.stride(2) && t.stride(0) == H * t.stride(1) &&
           aligned(t, 16) && t.scalar_type() == at::kBFloat16 &&
           avail_elems(t) * 2 < (1LL << 31) - 64;
  };
  const int64_t B = x.size(0), H = x.size(1);
  TORCH_CHECK(rows_ok(x, B, H), "aiko.conv3x3_rows_out: x must be [B, H, 80, >= 32] bf16 with uniformly strided rows");
  TORCH_CHECK(rows_ok(y, B, H) && y.size(3) == 32, "aiko.conv3x3_rows_out: y must be [B, H, 80, 32] bf16 (a slice is fine)");
  TORCH_CHECK(wimg.is_contiguous() && wimg.numel() == 9 * 32 * 32 && wimg.scalar_type() == at::kBFloat16,
              "aiko.conv3x3_rows_out: wimg must be the 9216-element bf16 image");
  const void* rptr = nullptr;
  int64_t ldr = 0;
  if (defined(res)) {
    check_cuda(*res, "res");
    TORCH_CHECK(rows_ok(*res, B, H), "aiko.conv3x3_rows_out: res must be [B, H, 80, >= 32] bf16 with uniformly strided rows");
    rptr = res->data_ptr();
    ldr = res->stride(2);
  }
  TORCH_CHECK((act & 15) <= 2 && (act & ~31) == 0, "aiko.conv3x3_rows_out: act none / relu / silu (+16: residual after)");
  const float* bptr = nullptr;
  if (defined(bias)) {
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
  const bool dual = defined(A2_opt);
  TORCH_CHECK(dual != (defined(R_opt)),
              "aiko.conv_chain_out: exactly one of R (identity residual) and A2 (fused projection shortcut)");
  const at::Tensor& R = dual ? *A2_opt : *R_opt;   // (validated by the dual branch below when dual)
  for (const at::Tensor* t : {&A, &W1, &b1, &R, (const at::Tensor*)&Y, &W2, &b2, (const at::Tensor*)&Z}) {
    check_cuda(*t, "conv_chain operand");
    TORCH_CHECK(t->is_contiguous() && aligned(*t, 16),
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
                  aligned(x, 16) && aligned(y, 8),
              "aiko.c2f_fused_out: NHWC views with 16-B aligned pixels");
  // optional in-place 2x upsample source for input channels [0, cu): xu [B, H/2, W/2, cu] (NHWC view)
  const void* xup = nullptr;
  int64_t ldxu = 0, cu = 0;
  if (defined(xu_opt)) {
    const at::Tensor& xu = *xu_opt;
    check_cuda(xu, "c2f upsample source");
    TORCH_CHECK(xu.scalar_type() == at::kBFloat16 && xu.dim() == 4 && xu.size(0) == B && 2 * xu.size(1) == H &&
                    2 * xu.size(2) == W && xu.stride(3) == 1 && xu.stride(1) == xu.size(2) * xu.stride(2) &&
                    xu.stride(0) == xu.size(1) * xu.stride(1) && xu.stride(2) % 8 == 0 &&
                    aligned(xu, 16),
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
                  aligned(x, 16) && aligned(y, 8),
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
                  aligned(x, 16),
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
                  aligned(y2, 16),
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
                  aligned(x, 16),
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
    TORCH_CHECK(t->is_contiguous() && aligned(*t, 16),
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
    TORCH_CHECK(t->is_contiguous() && aligned(*t, 16),
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
  check_cuda_all({&frames, &w, &out}, {"frames", "w", "out"});
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
  if (defined(bias)) {
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

// Fused 7x7/s2 stem conv + bias + ReLU + 3x3/s2/p1 max-pool (stem_pool.hip).  x: the zero-bordered
// [B, Hp, Wp, 4] preprocess buffer; w: [7, 64, 32] LDS image of the stem weights (16-byte chunks
// XOR-swizzled by channel >> 2, built by ops.conv.stem_pool); y: [B, Hm, Wm, 64] (slice ok).
void stem_pool_out(const at::Tensor& x, const at::Tensor& w, const at::Tensor& bias, at::Tensor& y,
                   int64_t Ho, int64_t Wo, int64_t variant) {
  check_cuda_all({&x, &w, &bias, &y}, {"x", "w", "bias", "y"});
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
  TORCH_CHECK(aligned(x, 16) && aligned(w, 16) && aligned(bias, 16),
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
  check_cuda_all({&frames, &w, &bias, &y}, {"frames", "w", "bias", "y"});
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
  TORCH_CHECK(aligned(frames, 4) && aligned(w, 16) && aligned(bias, 16),
              "aiko.stem_pool_u8_out: frames 4-byte, w / bias 16-byte aligned");
  const float m[3] = {(float)mean255[0], (float)mean255[1], (float)mean255[2]};
  check_launch(aiko_stem_pool_u8(frames.data_ptr(), w.data_ptr(), bias.data_ptr<float>(), y.data_ptr(), B, Hi, Wi,
                                 Ho, Wo, Hm, Wm, ldy, m, (int)variant, cur_stream()),
               "stem_pool_u8");
}

}  // namespace

TORCH_LIBRARY_IMPL(aiko, CUDA, m) {
  m.impl("conv_igemm_out", &conv_igemm_out);
  m.impl("conv3x3_patch_out", &conv3x3_patch_out);
  m.impl("conv3x3_patchw_out", &conv3x3_patchw_out);
  m.impl("conv3x3_rows_out", &conv3x3_rows_out);
  m.impl("conv_chain_out", &conv_chain_out);
  m.impl("c2f_fused_out", &c2f_fused_out);
  m.impl("c2f_bneck_out", &c2f_bneck_out);
  m.impl("conv_glds_tail_out", &conv_glds_tail_out);
  m.impl("conv_glds_tail_decode_out", &conv_glds_tail_decode_out);
  m.impl("bneck_fused_out", &bneck_fused_out);
  m.impl("conv3x3_exp_out", &conv3x3_exp_out);
  m.impl("stem_direct_out", &stem_direct_out);
  m.impl("stem_pool_out", &stem_pool_out);
  m.impl("stem_pool_u8_out", &stem_pool_u8_out);
}
