// Baseline JPEG decoding on the device (gfx950), the inverse of jpeg_ops.hip: one JPEG stream per row
// of ``data`` [B, cap], its length in ``nbytes`` [B], its header's descriptor in ``desc`` (one row per
// frame, or one row for all) -> tightly packed i420 / yuyv / i444 frames in ``raw`` [B, frame_bytes]
// and a status per frame.  Three launches, no host copy, no synchronisation, no global atomics, no
// float.  The rule, the descriptor and the workspace layout are stated in ops/jpeg_decode.py;
// ops/reference.py jpeg_decode_ref gives the same bits.
//
//   * jpeg_scan_kernel: one workgroup per frame walks [scan offset, nbytes - 2) in chunks of a byte
//     per thread; ballot and popcount give every RST marker its ordinal, the marker behind interval
//     i - 1 gives interval i its start.  Count, order and the EOI are checked here.
//   * jpeg_entropy_kernel: one lane per (frame, restart interval), the frame's descriptor in LDS; the
//     serial decoder of jpeg_decode_core.h writes int16 coefficients in zigzag order and the
//     interval's status to the workspace.  Lanes diverge inside a block and go on independently.
//   * jpeg_idct_kernel: passes of JD_CHUNK blocks; a thread per (block, column) dequantises and
//     transforms the columns, a thread per (block, row) the rows, and stores its eight samples with
//     one 8-byte store where the row lies inside the plane and is aligned, else by bytes; for yuyv
//     the samples go through LDS and a thread stores four pixels, Y and chroma interleaved.  The
//     first workgroup of a frame also ORs the interval statuses into ``status``.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_decode_core.h"
#include "aiko_api.h"

namespace aiko {

constexpr int JD_THREADS = 256;
constexpr int JD_WAVES = JD_THREADS / 64;
constexpr int JD_CHUNK = JD_THREADS / 8;              // blocks per pass: a thread per (block, column)
constexpr int JD_LANES = 64;                          // intervals per workgroup of the entropy kernel
constexpr int JD_MAX_W = 4096;
constexpr int JD_MAX_H = 65535;

// natural (row-major) index -> zigzag position: the inverse of ops.jpeg.ZIGZAG
__constant__ uint8_t JD_ZZ[64] = {
     0,  1,  5,  6, 14, 15, 27, 28,
     2,  4,  7, 13, 16, 26, 29, 42,
     3,  8, 12, 17, 25, 30, 41, 43,
     9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54,
    20, 22, 33, 38, 46, 51, 55, 60,
    21, 34, 37, 47, 50, 56, 59, 61,
    35, 36, 48, 49, 57, 58, 62, 63};

struct JpegDecodeArgs {
  const uint8_t* data;          // [B, cap]
  const int* nbytes;            // [B]
  const uint8_t* desc;          // [B or 1, JD_PLAN_BYTES]
  long desc_stride;             // JD_PLAN_BYTES, or 0 for one row
  long cap;
  int* scan_status;             // [B]
  int* starts;                  // [B, max_int]
  int* istatus;                 // [B, max_int]
  int16_t* coef;                // [B, nblocks, 64]
  uint8_t* raw;                 // [B, frame_bytes]
  int* status;                  // [B]
  long frame_bytes;
  int H, W, fmt;                // fmt: 1 i420, 2 i444, 3 yuyv
  int mx, mcus, nblocks, max_int;
};

// intervals of a frame by its own DRI
__device__ __forceinline__ int jd_intervals(int dri, int mcus) { return dri > 0 ? (mcus + dri - 1) / dri : 1; }

// Grid (B).  The frame's scan status and interval starts.
__global__ __launch_bounds__(JD_THREADS) void jpeg_scan_kernel(const JpegDecodeArgs a) {
  __shared__ int s_cnt[2][JD_WAVES];
  __shared__ int s_bad;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* plan = reinterpret_cast<const uint32_t*>(a.desc + (long)b * a.desc_stride);
  const int scan = (int)plan[JD_P_SCAN / 4], dri = (int)plan[JD_P_DRI / 4];
  const int n = a.nbytes[b];
  if (n < 1 || (long)n > a.cap || scan < 2 || scan > n - 2 || dri < 0 || jd_intervals(dri, a.mcus) > a.max_int) {
    if (tid == 0) a.scan_status[b] = JD_E_MARKER;     // uniform: every thread leaves
    return;
  }
  const int nint = jd_intervals(dri, a.mcus);
  const uint8_t* d = a.data + (long)b * a.cap;
  int* starts = a.starts + (long)b * a.max_int;
  const int hi = n - 2;                               // a marker pair (i, i + 1) lies in [scan, hi)
  if (tid == 0) s_bad = 0;
  int running = 0, bad = 0, parity = 0;
  for (int base = scan; base + 1 < hi; base += JD_THREADS) {
    const int i = base + tid;
    uint32_t m = 0;
    bool is = false;
    if (i + 1 < hi) {
      m = d[i + 1];
      is = d[i] == 0xff && (m & 0xf8u) == 0xd0u;
    }
    const uint64_t vote = __ballot(is);
    if (lane == 0) s_cnt[parity][wave] = __popcll(vote);
    __syncthreads();
    int before = running, total = 0;
#pragma unroll
    for (int w = 0; w < JD_WAVES; ++w) {
      const int c = s_cnt[parity][w];
      if (w < wave) before += c;
      total += c;
    }
    if (is) {
      const int ord = before + __popcll(vote & ((1ull << lane) - 1ull));
      if (ord < nint - 1) {
        starts[ord + 1] = i + 2;
        bad |= (int)(m & 7u) != (ord & 7);
      }
    }
    running += total;
    parity ^= 1;                                      // the other row is next written behind this barrier
  }
  __syncthreads();
  if (bad) atomicOr(&s_bad, 1);
  __syncthreads();
  if (tid == 0) {
    starts[0] = scan;
    const bool eoi = d[n - 2] == 0xff && d[n - 1] == 0xd9;
    a.scan_status[b] = (s_bad || running != nint - 1 || !eoi) ? JD_E_MARKER : 0;
  }
}

// Grid (ceil(max_int / JD_LANES), B), JD_LANES threads: lane = interval.
__global__ __launch_bounds__(JD_LANES) void jpeg_entropy_kernel(const JpegDecodeArgs a) {
  __shared__ uint32_t s_plan[JD_PLAN_WORDS];
  const int b = blockIdx.y, lane = threadIdx.x;
  const uint32_t* plan = reinterpret_cast<const uint32_t*>(a.desc + (long)b * a.desc_stride);
  for (int i = lane; i < JD_PLAN_WORDS; i += JD_LANES) s_plan[i] = plan[i];
  __syncthreads();
  if (a.scan_status[b] != 0) return;                  // the frame's markers are wrong: nothing is decoded
  const int dri = (int)s_plan[JD_P_DRI / 4];
  const int nint = jd_intervals(dri, a.mcus);         // <= max_int: the scan checked it
  const int i = blockIdx.x * JD_LANES + lane;
  if (i >= nint) return;
  const int* starts = a.starts + (long)b * a.max_int;
  const int start = starts[i];
  const int end = i + 1 < nint ? starts[i + 1] - 2 : a.nbytes[b] - 2;
  const int mcu0 = dri > 0 ? i * dri : 0;
  const int mcu1 = dri > 0 ? min(a.mcus, mcu0 + dri) : a.mcus;
  const int st = jd_interval(a.data + (long)b * a.cap, start, end, s_plan, a.fmt, mcu0, mcu1,
                             a.coef + (long)b * a.nblocks * 64);
  a.istatus[(long)b * a.max_int + i] = st;
}

// y[n] = sum_k M[k][n] x[k], M = ops.jpeg.DCT_MATRIX, with M[k][7 - n] = (-1)^k M[k][n] folded: integer
// sums are order-free, so these are the bits of the plain sum
__device__ __forceinline__ void jd_idct8(const int (&x)[8], int (&y)[8]) {
  constexpr int JD_DCT[64] = {
      2896,  2896,  2896,  2896,  2896,  2896,  2896,  2896,
      4017,  3406,  2276,   799,  -799, -2276, -3406, -4017,
      3784,  1567, -1567, -3784, -3784, -1567,  1567,  3784,
      3406,  -799, -4017, -2276,  2276,  4017,   799, -3406,
      2896, -2896, -2896,  2896,  2896, -2896, -2896,  2896,
      2276, -4017,   799,  3406, -3406,  -799,  4017, -2276,
      1567, -3784,  3784, -1567, -1567,  3784, -3784,  1567,
       799, -2276,  3406, -4017,  4017, -3406,  2276,  -799};
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    int e = 0, o = 0;
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
      e += JD_DCT[k * 8 + n] * x[k];
      o += JD_DCT[(k + 1) * 8 + n] * x[k + 1];
    }
    y[n] = e + o;
    y[7 - n] = e - o;
  }
}

// Grid (ceil(nblocks / JD_CHUNK), B).
__global__ __launch_bounds__(JD_THREADS) void jpeg_idct_kernel(const JpegDecodeArgs a) {
  __shared__ int16_t s_t[JD_CHUNK * 64];              // [block][row][column] behind the column pass
  __shared__ __attribute__((aligned(8))) uint8_t s_out[JD_CHUNK * 64];     // yuyv: [block][row][column] samples
  __shared__ uint8_t s_q[192];
  __shared__ int s_status;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int H = a.H, W = a.W, fmt = a.fmt;
  const int per = jd_blocks_per_mcu(fmt);
  const uint8_t* plan = a.desc + (long)b * a.desc_stride;
  if (tid < 192) s_q[tid] = plan[JD_P_Q + tid];
  if (tid == 0) s_status = 0;
  __syncthreads();

  const int blk = tid >> 3, k = blockIdx.x * JD_CHUNK + blk;
  const bool live = k < a.nblocks;
  const int mcu = k / per, sub = k - mcu * per;
  const int comp = jd_component(fmt, sub);
  // 1. columns: thread (block, column c)
  if (live) {
    const int c = tid & 7;
    const int16_t* cf = a.coef + ((long)b * a.nblocks + k) * 64;
    int x[8], y[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int n = r * 8 + c;
      const int v = (int)cf[JD_ZZ[n]] * (int)s_q[comp * 64 + n];
      x[r] = min(max(v, -2048), 2047);
    }
    jd_idct8(x, y);
#pragma unroll
    for (int i = 0; i < 8; ++i) s_t[blk * 64 + i * 8 + c] = (int16_t)((y[i] + 1024) >> 11);
  }
  __syncthreads();
  // 2. rows: thread (block, row r)
  const int r = tid & 7;
  uint64_t px8 = 0;                                   // the row's samples, the leftmost in the low byte
  if (live) {
    int x[8], y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = s_t[blk * 64 + r * 8 + j];
    jd_idct8(x, y);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int s = min(max(((y[j] + 16384) >> 15) + 128, 0), 255);
      px8 |= (uint64_t)s << (8 * j);
    }
  }
  uint8_t* frame = a.raw + (long)b * a.frame_bytes;
  if (fmt != 3) {
    if (live) {
      const int my_ = mcu / a.mx, mx_ = mcu - my_ * a.mx;
      int pw, ph, bx, by;
      long base;
      if (fmt == 1 && sub < 4) {
        pw = W; ph = H; base = 0;
        bx = mx_ * 2 + (sub & 1); by = my_ * 2 + (sub >> 1);
      } else if (fmt == 1) {
        pw = (W + 1) >> 1; ph = (H + 1) >> 1;
        base = (long)H * W + (long)(sub - 4) * pw * ph;
        bx = mx_; by = my_;
      } else {
        pw = W; ph = H; base = (long)sub * H * W;
        bx = mx_; by = my_;
      }
      const int py = by * 8 + r, px = bx * 8;
      if (py < ph && px < pw) {
        uint8_t* p = frame + base + (long)py * pw + px;
        if (px + 8 <= pw && (reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
          *reinterpret_cast<uint64_t*>(p) = px8;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (px + j < pw) p[j] = (uint8_t)(px8 >> (8 * j));
        }
      }
    }
  } else {
    // yuyv: an MCU is Y0 Y1 Cb Cr, JD_CHUNK / 4 whole MCUs per pass; thread (MCU m, row, quarter q) stores
    // the four pixels x0 .. x0 + 3 as Y U Y V Y U Y V
    if (live) *reinterpret_cast<uint64_t*>(&s_out[blk * 64 + r * 8]) = px8;
    __syncthreads();                                  // fmt is uniform
    const int m = tid >> 5, row = (tid >> 2) & 7, q = tid & 3;
    const int k0 = blockIdx.x * JD_CHUNK + m * 4;
    if (k0 < a.nblocks) {                             // nblocks is a multiple of 4: the whole MCU is there
      const int mc = k0 >> 2;
      const int my_ = mc / a.mx, mx_ = mc - my_ * a.mx;
      const int y = my_ * 8 + row, x0 = mx_ * 16 + q * 4;
      if (y < H && x0 < W) {
        const uint8_t* ys = &s_out[(m * 4 + (q >> 1)) * 64 + row * 8 + (q & 1) * 4];
        const uint8_t* us = &s_out[(m * 4 + 2) * 64 + row * 8 + q * 2];
        const uint8_t* vs = &s_out[(m * 4 + 3) * 64 + row * 8 + q * 2];
        const uint32_t lo = ys[0] | (uint32_t)us[0] << 8 | (uint32_t)ys[1] << 16 | (uint32_t)vs[0] << 24;
        const uint32_t hi = ys[2] | (uint32_t)us[1] << 8 | (uint32_t)ys[3] << 16 | (uint32_t)vs[1] << 24;
        uint8_t* p = frame + ((long)y * W + x0) * 2;
        if (x0 + 4 <= W && (reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
          *reinterpret_cast<uint64_t*>(p) = (uint64_t)hi << 32 | lo;
        } else {                                      // W is even: whole pairs
#pragma unroll
          for (int j = 0; j < 4; ++j) p[j] = (uint8_t)(lo >> (8 * j));
          if (x0 + 2 < W) {
#pragma unroll
            for (int j = 0; j < 4; ++j) p[4 + j] = (uint8_t)(hi >> (8 * j));
          }
        }
      }
    }
  }
  // 3. the frame's status, by its first workgroup
  if (blockIdx.x == 0) {
    int st = a.scan_status[b];
    if (st == 0) {
      const int dri = (int)reinterpret_cast<const uint32_t*>(plan)[JD_P_DRI / 4];
      const int nint = jd_intervals(dri, a.mcus);
      const int* is = a.istatus + (long)b * a.max_int;
      for (int i = tid; i < nint; i += JD_THREADS) st |= is[i];
    }
    if (st) atomicOr(&s_status, st);                  // LDS
    __syncthreads();
    if (tid == 0) a.status[b] = s_status;
  }
}

}  // namespace aiko

namespace {

// The launches' arguments, or false for a configuration they do not cover.  The workspace: int32
// [B] scan status, int32 [B, max_int] starts, int32 [B, max_int] interval statuses, padding to 16
// bytes, int16 [B, nblocks, 64] coefficients.
bool jpeg_decode_args(aiko::JpegDecodeArgs& a, const void* data, const int* nbytes, const void* desc, int desc_rows,
                      void* workspace, void* raw, int* status, int B, int H, int W, int fmt, long cap, int max_int) {
  using namespace aiko;
  if ((fmt != 1 && fmt != 2 && fmt != 3) || B < 1 || B > 65535 || H < 1 || H > JD_MAX_H || W < 1 || W > JD_MAX_W ||
      (fmt == 3 && (W & 1)) || cap < 1 || cap > INT32_MAX || (desc_rows != 1 && desc_rows != B) ||
      reinterpret_cast<uintptr_t>(workspace) % 16 || reinterpret_cast<uintptr_t>(desc) % 4)
    return false;
  const int mh = fmt == 1 ? 16 : 8, mw = fmt == 2 ? 8 : 16;
  const int my = (H + mh - 1) / mh, mx = (W + mw - 1) / mw;
  const long mcus = (long)my * mx;
  if (max_int < 1 || max_int > mcus) return false;
  const long ints = (long)B * (1 + 2L * max_int);
  a.data = static_cast<const uint8_t*>(data);
  a.nbytes = nbytes;
  a.desc = static_cast<const uint8_t*>(desc);
  a.desc_stride = desc_rows == 1 ? 0 : JD_PLAN_BYTES;
  a.cap = cap;
  a.scan_status = static_cast<int*>(workspace);
  a.starts = a.scan_status + B;
  a.istatus = a.starts + (long)B * max_int;
  a.coef = reinterpret_cast<int16_t*>(static_cast<uint8_t*>(workspace) + (4 * ints + 15) / 16 * 16);
  a.raw = static_cast<uint8_t*>(raw);
  a.status = status;
  const long ch = (H + 1) / 2, cw = (W + 1) / 2;
  a.frame_bytes = fmt == 1 ? (long)H * W + 2 * ch * cw : (fmt == 2 ? 3L * H * W : 2L * H * W);
  a.H = H; a.W = W; a.fmt = fmt;
  a.mx = mx; a.mcus = (int)mcus; a.nblocks = (int)mcus * jd_blocks_per_mcu(fmt); a.max_int = max_int;
  return true;
}

}  // namespace

// The entry points return -1 for a configuration the launches do not cover.  fmt: the codes of
// ops.yuv.FORMATS (1 i420, 2 i444, 3 yuyv); desc: desc_rows (1 or B) rows of ops.jpeg_decode.PLAN_BYTES,
// 4-byte aligned; workspace: ops.jpeg_decode.workspace_bytes, 16-byte aligned; max_int: the
// intervals per frame provided for, 1 .. MCUs of a frame.  ``pass``: 0 the marker scan, 1 the entropy
// decode, 2 the IDCT and the status.
extern "C" int aiko_jpeg_decode_pass(int pass, const void* data, const int* nbytes, const void* desc, int desc_rows,
                                     void* workspace, void* raw, int* status, int B, int H, int W, int fmt, long cap,
                                     int max_int, hipStream_t strm) {
  using namespace aiko;
  JpegDecodeArgs a;
  if (!jpeg_decode_args(a, data, nbytes, desc, desc_rows, workspace, raw, status, B, H, W, fmt, cap, max_int))
    return -1;
  if (pass == 0)
    jpeg_scan_kernel<<<dim3((unsigned)B), JD_THREADS, 0, strm>>>(a);
  else if (pass == 1)
    jpeg_entropy_kernel<<<dim3((unsigned)((max_int + JD_LANES - 1) / JD_LANES), (unsigned)B), JD_LANES, 0, strm>>>(a);
  else if (pass == 2)
    jpeg_idct_kernel<<<dim3((unsigned)((a.nblocks + JD_CHUNK - 1) / JD_CHUNK), (unsigned)B), JD_THREADS, 0, strm>>>(a);
  else
    return -1;
  return (int)hipGetLastError();
}

// One decode: the three passes on ``strm``.
extern "C" int aiko_jpeg_decode(const void* data, const int* nbytes, const void* desc, int desc_rows, void* workspace,
                                void* raw, int* status, int B, int H, int W, int fmt, long cap, int max_int,
                                hipStream_t strm) {
  for (int pass = 0; pass < 3; ++pass) {
    const int rc = aiko_jpeg_decode_pass(pass, data, nbytes, desc, desc_rows, workspace, raw, status, B, H, W, fmt,
                                         cap, max_int, strm);
    if (rc) return rc;
  }
  return 0;
}
