// Voice activity (gfx950): did anybody speak in this chunk, and when?  16 kHz mono fp32 chunks
// [B, n] (batch row b is stream b) against a per-stream state of 8 ints that stays in HBM between
// chunks (noise floor, onset and hangover counters, time since the last speech frame) -> a mask per
// frame of 10, 20 or 30 ms, its runs as segments, and one ``silent`` flag per stream that the
// decoder takes as its ``done``.  Two launches per chunk, no host copy, no synchronisation.  The
// rule is stated in ops/vad.py; after one exact fp32 scaling it is all integer, and ops/reference.py
// voice_activity_ref gives the same bits.
//
//   * vad_frames_kernel: the memory-bound part.  Every sample is read once, by one wave64 per
//     frame: lanes quantise to 16 bits, add the squares in 64 bits and count the sign changes
//     against the sample before (the lane below's last, by shuffle; lane 63's of the pass before);
//     an xor-shuffle reduction, then lane 0 writes the frame's level and zero crossings.
//   * vad_stream_kernel: one workgroup per stream.  The level and zero-crossing rows go into LDS,
//     one wave walks the frames with wave-uniform state (the floor's recursion is serial by nature),
//     then all threads write the mask and find the runs: ballots of starts and ends per 64 frames, a
//     wave scan over the at most 64 words for the ordinals.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aiko_api.h"

namespace aiko {

constexpr int VA_WAVES = 4;                           // frames per workgroup of the frame pass
constexpr int VA_THREADS = 64 * VA_WAVES;
constexpr int VA_MAX_FRAME = 480;
constexpr int VA_MAX_F = 4096;                        // frames per call and stream
constexpr int VA_WORDS = VA_MAX_F / 64;               // ballot words of a stream's mask
constexpr int VA_MAX_SEG = 64;
constexpr int VA_CAP = 1 << 30;                       // where run and since stop counting
constexpr int VA_MAX_LEVEL = 1023;                    // a floor read from the state is held to 0 .. 1023 level units
constexpr int VS_THREADS = 256;
constexpr int VS_WAVES = VS_THREADS / 64;
static_assert(VA_WORDS <= 64, "one wave scans the words");

struct VadFrameArgs {
  const float* audio;           // [B, F * frame]
  int* level;                   // [B, F]
  int* zc;                      // [B, F]
  int F, frame;
};

// step 1 of the rule: x * 2^15 is exact, NaN -> 0, +-inf clamp, round half to even
__device__ __forceinline__ int va_quantise(float x) {
  const float v = x * 32768.0f;
  if (v != v) return 0;
  return (int)rintf(fminf(fmaxf(v, -32768.0f), 32767.0f));
}

// step 3: 16 * (floor(log2 E) + 1) + the next four bits of E, 0 for E = 0
__device__ __forceinline__ int va_level(uint64_t E) {
  if (E == 0) return 0;
  const int p = 63 - __clzll((long long)E);
  const int mant = (int)((p >= 4 ? E >> (p - 4) : E << (4 - p)) & 15u);
  return 16 * (p + 1) + mant;
}

// Grid (ceil(F / VA_WAVES), B), one wave per frame; a lane owns PER adjacent samples per pass (VEC:
// one float4; a frame is 40, 80 or 120 of them, and 16-byte aligned when the row is), the passes
// cover the frame 64 * PER samples at a time.
template <bool VEC>
__global__ __launch_bounds__(VA_THREADS) void vad_frames_kernel(const VadFrameArgs a) {
  constexpr int PER = VEC ? 4 : 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * VA_WAVES + wave, b = blockIdx.y;
  if (f >= a.F) return;                               // a whole wave: the shuffles below stay uniform
  const float* x = a.audio + ((long)b * a.F + f) * a.frame;
  const int items = a.frame / PER;                    // 4 | frame

  uint64_t E = 0;
  int z = 0;
  int last = 0;                                       // lane 63: the last sample of the pass before
  for (int i0 = 0; i0 < items; i0 += 64) {            // at most ceil(frame / 64) passes
    const int i = i0 + lane;
    const bool in = i < items;
    int q[PER];
    if constexpr (VEC) {
      const float4 v = in ? reinterpret_cast<const float4*>(x)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      q[0] = va_quantise(v.x); q[1] = va_quantise(v.y); q[2] = va_quantise(v.z); q[3] = va_quantise(v.w);
    } else {
      q[0] = in ? va_quantise(x[i]) : 0;
    }
    int prev = __shfl_up(q[PER - 1], 1);              // the sample before this lane's first
    const int carry = __shfl(last, 63);
    if (lane == 0) prev = carry;
    if (in) {
      if (i > 0) z += (q[0] < 0) != (prev < 0);
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        E += (uint64_t)((int64_t)q[k] * q[k]);
        if (k > 0) z += (q[k] < 0) != (q[k - 1] < 0);
      }
    }
    last = q[PER - 1];
  }
  uint32_t lo = (uint32_t)E, hi = (uint32_t)(E >> 32);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t o = ((uint64_t)(uint32_t)__shfl_xor((int)hi, d) << 32) | (uint32_t)__shfl_xor((int)lo, d);
    E += o;
    lo = (uint32_t)E; hi = (uint32_t)(E >> 32);
    z += __shfl_xor(z, d);
  }
  if (lane == 0) {
    const long o = (long)b * a.F + f;
    a.level[o] = va_level(E);
    a.zc[o] = z;
  }
}

struct VadStreamArgs {
  const int* level;             // [B, F]
  const int* zc;                // [B, F]
  const int* state;             // [B, 8]: floor, seen, run, quiet, on, since, 0, 0
  int* state_out;
  uint8_t* mask;                // [B, F]
  int* seg;                     // [B, max_seg, 2]
  int* count;                   // [B]
  int* speech;                  // [B]
  int* silent;                  // [B]
  int F, max_seg;
  int thr8;                     // threshold << 8
  int min_level, up_shift, speech_shift, down_shift, warmup, attack, hang, max_zc, window;
};

__device__ __forceinline__ int va_wave_scan(int v, int lane) {    // inclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// Grid B, one workgroup per stream.
__global__ __launch_bounds__(VS_THREADS) void vad_stream_kernel(const VadStreamArgs a) {
  __shared__ int s_level[VA_MAX_F];
  __shared__ int s_zc[VA_MAX_F];
  __shared__ uint8_t s_mask[VA_MAX_F];
  __shared__ unsigned long long s_start[VA_WORDS], s_end[VA_WORDS];
  __shared__ int s_on[VA_WORDS];                      // mask bits per word
  __shared__ int s_sbase[VA_WORDS], s_ebase[VA_WORDS];     // starts / ends before the word
  __shared__ int s_total[2];                          // runs, speech frames

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int F = a.F;                                  // 1..VA_MAX_F: the host refuses the rest
  const long row = (long)b * F;
  for (int f = tid; f < F; f += VS_THREADS) {
    s_level[f] = a.level[row + f];
    s_zc[f] = a.zc[row + f];
  }
  __syncthreads();

  // Step 5, frame by frame: the recursion is serial, so one wave runs it with every lane computing
  // the same values.  64 frames at a time sit in two registers, one frame per lane, and come out by
  // readlane, so that the state and all its arithmetic are wave-uniform (scalar registers, the scalar
  // ALU) and no LDS read waits inside the recursion; the mask goes back one bit per lane.
  if (wave == 0) {
    const int* st = a.state + b * 8;
    int floor_ = min(max(st[0], 0), VA_MAX_LEVEL << 8);
    int s = max(st[1], 0);
    int run = min(max(st[2], 0), VA_CAP), quiet = max(st[3], 0), on = st[4] != 0;
    int since = min(max(st[5], 0), VA_CAP);
    if (s == 0) {                                     // the empty state, whatever the columns hold
      run = 0; quiet = 0; on = 0; since = VA_CAP;
    }
    for (int f0 = 0; f0 < F; f0 += 64) {
      const int fl = f0 + lane;
      const int vl = fl < F ? s_level[fl] : 0, vz = fl < F ? s_zc[fl] : 0;
      const int nf = min(64, F - f0);
      unsigned long long word = 0;
      for (int j = 0; j < nf; ++j) {
        const int level = __builtin_amdgcn_readlane(vl, j), z = __builtin_amdgcn_readlane(vz, j);
        const int cur = level << 8;                   // <= 639 << 8, floor_ in 0 .. 1023 << 8: no overflow
        if (s == 0) floor_ = cur;
        const bool raw = s >= a.warmup && level >= a.min_level && cur - floor_ > a.thr8 && z <= a.max_zc;
        if (s > 0) {
          const int k = cur < floor_ ? a.down_shift : raw ? a.speech_shift : a.up_shift;
          const int half = k ? 1 << (k - 1) : 0;
          floor_ += (cur - floor_ + half) >> k;
        }
        run = raw ? min(run + 1, VA_CAP) : 0;
        if (!on) {
          if (run >= a.attack) { on = 1; quiet = 0; }
        } else {
          if (raw) {
            quiet = 0;
          } else if (quiet >= a.hang) {               // quiet + 1 > hang
            on = 0; quiet = 0;
          } else {
            ++quiet;
          }
        }
        word |= (unsigned long long)on << j;
        since = on ? 0 : min(since + 1, VA_CAP);
        s = s == INT32_MAX ? s : s + 1;
      }
      if (fl < F) s_mask[fl] = (uint8_t)((word >> lane) & 1ull);
    }
    if (lane == 0) {
      int* so = a.state_out + b * 8;
      so[0] = floor_; so[1] = s; so[2] = run; so[3] = quiet; so[4] = on; so[5] = since; so[6] = 0; so[7] = 0;
      a.silent[b] = since >= a.window ? 1 : 0;
    }
  }
  __syncthreads();

  // the mask out, and per word of 64 frames the ballots of run starts and run ends (an end is the
  // run's last frame; the row holds one past it)
  const int words = (F + 63) >> 6;
  for (int w = wave; w < words; w += VS_WAVES) {      // uniform in a wave
    const int f = w * 64 + lane;
    const bool in = f < F;
    const bool m = in && s_mask[f];
    if (in) a.mask[row + f] = m ? 1 : 0;
    const bool st = m && (f == 0 || !s_mask[f - 1]);
    const bool en = m && (f == F - 1 || !s_mask[f + 1]);
    const unsigned long long bs = __ballot(st), be = __ballot(en), bm = __ballot(m);
    if (lane == 0) {
      s_start[w] = bs; s_end[w] = be; s_on[w] = __popcll(bm);
    }
  }
  __syncthreads();
  if (wave == 0) {                                    // ordinals: starts and ends before each word
    const bool in = lane < words;
    const int ns = in ? __popcll(s_start[lane]) : 0, ne = in ? __popcll(s_end[lane]) : 0;
    const int is = va_wave_scan(ns, lane), ie = va_wave_scan(ne, lane);
    const int sp = va_wave_scan(in ? s_on[lane] : 0, lane);
    if (in) {
      s_sbase[lane] = is - ns; s_ebase[lane] = ie - ne;
    }
    if (lane == 63) {
      s_total[0] = is; s_total[1] = sp;
    }
  }
  __syncthreads();
  const int n = min(s_total[0], a.max_seg);           // rows written: the k-th end closes the k-th start
  int* rows = a.seg + (long)b * a.max_seg * 2;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int w = wave; w < words; w += VS_WAVES) {
    const unsigned long long bs = s_start[w], be = s_end[w];
    const int f = w * 64 + lane;
    if ((bs >> lane) & 1ull) {
      const int k = s_sbase[w] + __popcll(bs & below);
      if (k < n) rows[2 * k] = f;
    }
    if ((be >> lane) & 1ull) {
      const int k = s_ebase[w] + __popcll(be & below);
      if (k < n) rows[2 * k + 1] = f + 1;
    }
  }
  for (int i = 2 * n + tid; i < 2 * a.max_seg; i += VS_THREADS) rows[i] = 0;
  if (tid == 0) {
    a.count[b] = n;
    a.speech[b] = s_total[1];
  }
}

}  // namespace aiko

namespace {

bool vad_shape(int B, int F, int frame) {
  return (frame == 160 || frame == 320 || frame == 480) && B >= 1 && B <= 65535 && F >= 1 && F <= aiko::VA_MAX_F;
}

bool shift_ok(int k) { return k >= 0 && k <= 16; }

}  // namespace

// The entry points return -1 for a configuration the launches do not cover.
// The frame pass: audio fp32 [B, F * frame] -> level int32 [B, F], zc int32 [B, F].
extern "C" int aiko_vad_frames(const float* audio, int* level, int* zc, int B, int F, int frame, hipStream_t stream) {
  if (!vad_shape(B, F, frame)) return -1;
  aiko::VadFrameArgs c;
  c.audio = audio; c.level = level; c.zc = zc; c.F = F; c.frame = frame;
  const dim3 grid((unsigned)((F + aiko::VA_WAVES - 1) / aiko::VA_WAVES), (unsigned)B);
  if (reinterpret_cast<uintptr_t>(audio) % 16 == 0)   // a row is F * frame * 4 bytes, 16 | frame * 4
    aiko::vad_frames_kernel<true><<<grid, aiko::VA_THREADS, 0, stream>>>(c);
  else
    aiko::vad_frames_kernel<false><<<grid, aiko::VA_THREADS, 0, stream>>>(c);
  return (int)hipGetLastError();
}

// The stream pass: level, zc int32 [B, F] and state int32 [B, 8] -> state_out, mask uint8 [B, F], seg
// int32 [B, max_seg, 2], count, speech, silent int32 [B].
extern "C" int aiko_vad_stream(const int* level, const int* zc, const int* state, int* state_out, void* mask, int* seg,
                               int* count, int* speech, int* silent, int B, int F, int frame, int threshold,
                               int min_level, int up_shift, int speech_shift, int down_shift, int warmup, int attack,
                               int hang, int max_zc, int window, int max_seg, hipStream_t stream) {
  if (!vad_shape(B, F, frame) || threshold < 0 || threshold > 1023 || min_level < 0 || min_level > 1023 ||
      !shift_ok(up_shift) || !shift_ok(speech_shift) || !shift_ok(down_shift) || warmup < 1 || attack < 1 ||
      hang < 0 || max_zc < 0 || max_zc > aiko::VA_MAX_FRAME - 1 || window < 1 || max_seg < 1 ||
      max_seg > aiko::VA_MAX_SEG)
    return -1;
  aiko::VadStreamArgs r;
  r.level = level; r.zc = zc; r.state = state; r.state_out = state_out;
  r.mask = static_cast<uint8_t*>(mask);
  r.seg = seg; r.count = count; r.speech = speech; r.silent = silent;
  r.F = F; r.max_seg = max_seg;
  r.thr8 = threshold << 8;
  r.min_level = min_level; r.up_shift = up_shift; r.speech_shift = speech_shift; r.down_shift = down_shift;
  r.warmup = warmup; r.attack = attack; r.hang = hang; r.max_zc = max_zc; r.window = window;
  aiko::vad_stream_kernel<<<dim3((unsigned)B), aiko::VS_THREADS, 0, stream>>>(r);
  return (int)hipGetLastError();
}

// One step: both passes on ``stream``, nothing launched unless both are covered.
extern "C" int aiko_voice_activity(const float* audio, const int* state, int* state_out, int* level, int* zc, void* mask,
                                   int* seg, int* count, int* speech, int* silent, int B, int F, int frame,
                                   int threshold, int min_level, int up_shift, int speech_shift, int down_shift,
                                   int warmup, int attack, int hang, int max_zc, int window, int max_seg,
                                   hipStream_t stream) {
  if (threshold < 0 || threshold > 1023 || min_level < 0 || min_level > 1023 || !shift_ok(up_shift) ||
      !shift_ok(speech_shift) || !shift_ok(down_shift) || warmup < 1 || attack < 1 || hang < 0 || max_zc < 0 ||
      max_zc > aiko::VA_MAX_FRAME - 1 || window < 1 || max_seg < 1 || max_seg > aiko::VA_MAX_SEG)
    return -1;
  const int rc = aiko_vad_frames(audio, level, zc, B, F, frame, stream);
  return rc ? rc
            : aiko_vad_stream(level, zc, state, state_out, mask, seg, count, speech, silent, B, F, frame, threshold,
                              min_level, up_shift, speech_shift, down_shift, warmup, attack, hang, max_zc, window,
                              max_seg, stream);
}
