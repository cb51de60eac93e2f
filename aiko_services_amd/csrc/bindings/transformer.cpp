// torch.ops.aiko.*: FP8 GEMM, split-K linear, attention and the Whisper decoder's step.
// Each operator validates shapes / dtypes / devices on the host (checks.h holds the shared
// checks) and launches on the caller's current HIP stream.
#include "checks.h"

namespace {

int64_t row_pitch(const at::Tensor& t, int64_t cols, const char* op, const char* name) {
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1 && t.size(1) == cols && t.stride(0) >= cols,
              "aiko.", op, ": ", name, " must be a row-major [rows, ", cols, "] matrix (row slices / column slices allowed)");
  TORCH_CHECK(aligned(t, 16) && (t.stride(0) * t.element_size()) % 16 == 0,
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
  const bool mx_in = defined(amx);
  const bool mx_out = defined(yq);
  const float* sap = nullptr;
  if (!mx_in) {
    TORCH_CHECK(defined(sa_opt), "aiko.gemm_fp8_out: sa needed without amx");
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
  if (defined(y_opt)) {
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
    TORCH_CHECK(defined(ysc), "aiko.gemm_fp8_out: yq needs ysc");
    check_cuda(*ysc, "ysc");
    TORCH_CHECK(yq->element_size() == 1 && yq->size(0) == M && N % 128 == 0, "aiko.gemm_fp8_out: yq uint8 [M, N], N % 128 == 0");
    ldq = row_pitch(*yq, N, "gemm_fp8_out", "yq");
    TORCH_CHECK(ysc->element_size() == 1 && ysc->dim() == 3 && ysc->size(0) == N / 128 && ysc->size(1) >= M &&
                    ysc->size(2) == 4 && ysc->is_contiguous(),
                "aiko.gemm_fp8_out: ysc must be uint8 [N/128, rows >= M, 4]");
    TORCH_CHECK(!defined(res), "aiko.gemm_fp8_out: no residual with MX output");
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
  if (defined(bias)) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == N && bias->is_contiguous(), "aiko.gemm_fp8_out: bias fp32 [N]");
    bp = bias->data_ptr<float>();
  }
  const void* rp = nullptr;
  int64_t ldr = 0;
  if (defined(res)) {
    check_cuda(*res, "residual");
    TORCH_CHECK(res->scalar_type() == at::kBFloat16 && res->size(0) == M, "aiko.gemm_fp8_out: residual bf16 [M, N]");
    ldr = row_pitch(*res, N, "gemm_fp8_out", "residual");
    rp = res->data_ptr();
  }
  TORCH_CHECK(lda * M < INT_MAX * 2L, "aiko.gemm_fp8_out: A too large");
  const void* zp = nullptr;
  if (variant >= 1) {
    TORCH_CHECK(defined(zero) && zero->is_cuda() && zero->nbytes() >= 16 &&
                    aligned(*zero, 16),
                "aiko.gemm_fp8_out: the LDS-DMA variants need a zero page tensor (>= 16 B)");
    TORCH_CHECK(aligned(a, 16) && aligned(b, 16),
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
  if (defined(gamma)) {
    TORCH_CHECK(defined(beta), "aiko.rownorm_quant_out: gamma needs beta");
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
  if (defined(yb)) {
    check_cuda(*yb, "yb");
    TORCH_CHECK(yb->scalar_type() == at::kBFloat16 && yb->size(0) == M, "aiko.rownorm_quant_out: yb bf16 [M, D]");
    ldyb = row_pitch(*yb, D, "rownorm_quant_out", "yb");
    yp = yb->data_ptr();
  }
  void* qp = nullptr;
  float* sp = nullptr;
  int64_t ldq = 0;
  if (defined(q)) {
    TORCH_CHECK(defined(qs), "aiko.rownorm_quant_out: q needs qs");
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
                  aligned(x, 16) && aligned(w, 16) &&
                  aligned(y, 8) && aligned(part, 16),
              "aiko.linear_splitk_out: 16-B aligned operand rows");
  TORCH_CHECK(part.numel() >= S * M * N, "aiko.linear_splitk_out: part too small");
  const float* bp = nullptr;
  if (defined(bias)) {
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
  if (defined(work)) {
    check_cuda(*work, "work");
    TORCH_CHECK(work->is_contiguous() && aligned(*work, 256),
                "aiko.attn_fwd_out: work must be a contiguous, 256-byte aligned (zero-initialised) buffer");
    wp = work->data_ptr();
    wb = (long)(work->numel() * work->element_size());
  }
  // MX-fp8 output (ops.transformer.mx_buffers layout): e4m3 [B*Tpad, >= H*64] + E8M0 scales
  // [H*64/128][rows >= B*Tpad][4]; o is then not written
  void* qp = nullptr;
  void* sp = nullptr;
  int ldoq = 0, osr = 0;
  if (defined(oq)) {
    TORCH_CHECK(defined(osc), "aiko.attn_fwd_out: oq needs osc");
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

// ---- decoder step ops (decode_ops.hip) ----------------------------------------------------------

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
  TORCH_CHECK(aligned(x, 16), "aiko.embed_tokens_out: x alignment");
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
  const bool app = defined(pos);
  for (const at::Tensor* t : {&q, (const at::Tensor*)&k, (const at::Tensor*)&v, (const at::Tensor*)&o}) {
    check_cuda(*t, "q/k/v/o");
    TORCH_CHECK(t->scalar_type() == at::kBFloat16 && t->dim() == 2, "aiko.attn_decode_out: bf16 2-D tensors required");
    row_pitch(*t, H * 64, "attn_decode_out", "q/k/v/o");
    TORCH_CHECK(aligned(*t, 16), "aiko.attn_decode_out: 16-byte alignment");
  }
  TORCH_CHECK(q.size(0) == B && o.size(0) == B, "aiko.attn_decode_out: q/o need B rows");
  TORCH_CHECK(k.size(0) == B * S && v.size(0) == B * S, "aiko.attn_decode_out: k/v need B*S rows");
  const void *kn = nullptr, *vn = nullptr;
  int64_t ldnew = 0;
  const int* pp = nullptr;
  if (app) {
    check_i32(*pos, 1, "pos");
    pp = pos->data_ptr<int>();
    TORCH_CHECK(defined(knew) && defined(vnew),
                "aiko.attn_decode_out: append mode needs knew and vnew");
    for (const at::Tensor* t : {&*knew, &*vnew}) {
      check_cuda(*t, "knew/vnew");
      TORCH_CHECK(t->scalar_type() == at::kBFloat16 && t->size(0) == B &&
                      aligned(*t, 16),
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
  TORCH_CHECK(aligned(x, 16) && aligned(w, 16),
              "aiko.dec_linear_out: x / w 16-byte alignment");
  const int64_t ldx = row_pitch(x, K, "dec_linear_out", "x");
  TORCH_CHECK(y.size(0) == M, "aiko.dec_linear_out: y [M, N]");
  const int64_t ldy = row_pitch(y, N, "dec_linear_out", "y");
  const float *g = nullptr, *be = nullptr, *bp = nullptr;
  if (defined(gamma)) {
    TORCH_CHECK(defined(beta), "aiko.dec_linear_out: gamma needs beta");
    for (const at::Tensor* t : {&*gamma, &*beta}) {
      check_cuda(*t, "gamma/beta");
      TORCH_CHECK(t->scalar_type() == at::kFloat && t->numel() == K && t->is_contiguous(), "aiko.dec_linear_out: gamma/beta fp32 [K]");
    }
    g = gamma->data_ptr<float>();
    be = beta->data_ptr<float>();
  }
  if (defined(bias)) {
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == N && bias->is_contiguous(), "aiko.dec_linear_out: bias fp32 [N]");
    bp = bias->data_ptr<float>();
  }
  const void* rp = nullptr;
  int64_t ldr = 0;
  if (defined(res)) {
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
                  aligned(logits, 16),
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

TORCH_LIBRARY_IMPL(aiko, CUDA, m) {
  m.impl("gemm_fp8_out", &gemm_fp8_out);
  m.impl("rownorm_quant_out", &rownorm_quant_out);
  m.impl("linear_splitk_out", &linear_splitk_out);
  m.impl("attn_fwd_out", &attn_fwd_out);
  m.impl("embed_tokens_out", &embed_tokens_out);
  m.impl("attn_decode_out", &attn_decode_out);
  m.impl("dec_linear_out", &dec_linear_out);
  m.impl("argmax_step_out", &argmax_step_out);
}
