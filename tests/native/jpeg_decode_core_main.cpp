// The serial JPEG decoder of csrc/kernels/jpeg_decode_core.h on the CPU, as a program of its own so that
// the host compiler's sanitizers see every read and store (tests/test_jpeg_decode_core_native.py builds
// it with -fsanitize=address,undefined and runs it as a process).
//
//   jpeg_decode_core_main DIR N CAP H W FMT
//
// reads DIR/data.bin (uint8 [N, CAP]), DIR/nbytes.bin (int32 [N]) and DIR/desc.bin (uint8 [N, 1744]) and
// writes DIR/coef.bin (int16 [N, blocks, 64], zeros where nothing was decoded) and DIR/status.bin (int32
// [N]).  Every frame's row is copied into an allocation of exactly nbytes bytes, and its coefficients
// are decoded into one of exactly blocks * 64 values, so that a read or a store outside either is the
// sanitizer's to report.  FMT: 1 i420, 2 i444, 3 yuyv.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "jpeg_decode_core.h"

namespace {

bool read_file(const std::string& path, void* dst, size_t bytes) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  const size_t got = fread(dst, 1, bytes, f);
  fclose(f);
  return got == bytes;
}

bool write_file(const std::string& path, const void* src, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const size_t put = fwrite(src, 1, bytes, f);
  return fclose(f) == 0 && put == bytes;
}

}  // namespace

int main(int argc, char** argv) {
  using namespace aiko;
  if (argc != 7) {
    fprintf(stderr, "usage: %s DIR N CAP H W FMT\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const long N = atol(argv[2]), cap = atol(argv[3]);
  const int H = atoi(argv[4]), W = atoi(argv[5]), fmt = atoi(argv[6]);
  if (N < 1 || cap < 1 || H < 1 || W < 1 || fmt < 1 || fmt > 3) return 2;
  const int mh = fmt == 1 ? 16 : 8, mw = fmt == 2 ? 8 : 16;
  const int mcus = ((H + mh - 1) / mh) * ((W + mw - 1) / mw);
  const long nblocks = (long)mcus * jd_blocks_per_mcu(fmt);
  std::vector<uint8_t> data((size_t)(N * cap)), desc((size_t)(N * JD_PLAN_BYTES));
  std::vector<int32_t> nbytes((size_t)N), status((size_t)N, 0);
  std::vector<int16_t> coef((size_t)(N * nblocks * 64), 0);
  if (!read_file(dir + "/data.bin", data.data(), data.size()) ||
      !read_file(dir + "/nbytes.bin", nbytes.data(), 4 * nbytes.size()) ||
      !read_file(dir + "/desc.bin", desc.data(), desc.size())) {
    fprintf(stderr, "cannot read the inputs in %s\n", dir.c_str());
    return 2;
  }
  std::vector<int> starts((size_t)mcus);
  for (long f = 0; f < N; ++f) {
    const int n = nbytes[f];
    // exact allocations: the stream's bytes, the descriptor's words, the frame's coefficients
    const size_t len = n > 0 && n <= cap ? (size_t)n : 1;
    uint8_t* d = static_cast<uint8_t*>(malloc(len));
    uint32_t* plan = static_cast<uint32_t*>(malloc(JD_PLAN_BYTES));
    int16_t* out = static_cast<int16_t*>(aligned_alloc(16, (size_t)nblocks * 128));
    memcpy(d, data.data() + f * cap, len);
    memcpy(plan, desc.data() + f * JD_PLAN_BYTES, JD_PLAN_BYTES);
    memset(out, 0, (size_t)nblocks * 128);
    int count = 0;
    int st = jd_scan_serial(d, n, cap, plan, mcus, mcus, starts.data(), &count);
    if (st == 0) {
      const int dri = (int)plan[JD_P_DRI / 4];
      for (int i = 0; i < count; ++i) {
        const int end = i + 1 < count ? starts[i + 1] - 2 : n - 2;
        const int mcu0 = dri > 0 ? i * dri : 0;
        const int mcu1 = dri > 0 ? (mcu0 + dri < mcus ? mcu0 + dri : mcus) : mcus;
        st |= jd_interval(d, starts[i], end, plan, fmt, mcu0, mcu1, out);
      }
    }
    status[f] = st;
    memcpy(coef.data() + f * nblocks * 64, out, (size_t)nblocks * 128);
    free(out);
    free(plan);
    free(d);
  }
  if (!write_file(dir + "/coef.bin", coef.data(), 2 * coef.size()) ||
      !write_file(dir + "/status.bin", status.data(), 4 * status.size())) {
    fprintf(stderr, "cannot write the outputs in %s\n", dir.c_str());
    return 2;
  }
  return 0;
}
