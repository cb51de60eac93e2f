// torch.ops.aiko.*: audio: resampling, voice activity, spectrum analysis and the log-mel front end.
// Each operator validates shapes / dtypes / devices on the host (checks.h holds the shared
// checks) and launches on the caller's current HIP stream.
#include "checks.h"

namespace {

// out [B, n_in L / M], hist_out [B, T-1] <- pcm [B, n_in, C] (int16 or fp32, interleaved), the
// stream's previous T-1 mono samples hist [B, T-1] and the polyphase taps filt [L, T]
// (resample_ops.hip; the arithmetic is in ops/audio.py)
void resample_out(const at::Tensor& pcm, const at::Tensor& hist, const at::Tensor& filt, int64_t L, int64_t M,
                  at::Tensor& out, at::Tensor& hist_out) {
  const at::Tensor* ins[3] = {&pcm, &hist, &filt};
  const char* in_names[3] = {"pcm", "hist", "filt"};
  const at::Tensor* outs[2] = {&out, &hist_out};
  const char* out_names[2] = {"out", "hist_out"};
  check_cuda_all(ins, in_names);
  check_cuda_all(outs, out_names);
  check_same_device(ins, outs, "resample_out");
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
  check_no_overlap(outs, out_names, ins, in_names, "resample_out");
  check_launch(aiko_resample(pcm.data_ptr(), pcm.scalar_type() == at::kFloat ? 1 : 0, hist.data_ptr<float>(),
                             filt.data_ptr<float>(), out.data_ptr<float>(), hist_out.data_ptr<float>(), (int)B,
                             (long)n_in, (int)C, (int)L, (int)M, (int)T, cur_stream()),
               "resample");
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
  check_cuda_all(ins, in_names);
  check_cuda_all(outs, out_names);
  check_same_device(ins, outs, "voice_activity_out");
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
  check_no_overlap(outs, out_names, ins, in_names, "voice_activity_out");
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
  check_cuda_all(ins, in_names);
  check_cuda_all(outs, out_names);
  check_same_device(ins, outs, "spectrum_out");
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
  TORCH_CHECK(aligned(twiddle, 8), "aiko.spectrum_out: twiddle 8-byte aligned "
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
  check_no_overlap(outs, out_names, ins, in_names, "spectrum_out");
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
  const at::Tensor* ins[4] = {&peak_bins, &peak_amplitudes, &peak_counts, &bin_px};
  const char* in_names[4] = {"peak_bins", "peak_amplitudes", "peak_counts", "bin_px"};
  check_cuda_all(ins, in_names);
  check_cuda(image, "image");
  check_same_device(ins, {&image}, "spectrum_graph_out");
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
  check_no_overlap({&image}, {"image"}, ins, in_names, "spectrum_graph_out");
  check_launch(aiko_spectrum_graph(peak_bins.data_ptr<int>(), peak_amplitudes.data_ptr<float>(),
                                   peak_counts.data_ptr<int>(), bin_px.data_ptr<int>(), image.data_ptr(), (int)B, (int)H,
                                   (int)W, (int)bin_px.size(0), (int)max_peaks, y_max, (int)color[0], (int)color[1],
                                   (int)color[2], cur_stream()),
               "spectrum_graph");
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

}  // namespace

TORCH_LIBRARY_IMPL(aiko, CUDA, m) {
  m.impl("resample_out", &resample_out);
  m.impl("voice_activity_out", &voice_activity_out);
  m.impl("spectrum_out", &spectrum_out);
  m.impl("spectrum_graph_out", &spectrum_graph_out);
  m.impl("logmel_out", &logmel_out);
}
