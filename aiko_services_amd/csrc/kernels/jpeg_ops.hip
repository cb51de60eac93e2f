// Baseline JPEG on the device (gfx950): tightly packed planar i420 / i444 frames [B, frame_bytes] ->
// one complete JFIF stream per frame in ``stream`` [B, cap], its length in ``nbytes`` [B].  Two
// launches, no host copy, no synchronisation, no global atomics.  The rule (integer DCT, libjpeg's
// quantiser scaling, Annex K's Huffman tables, one restart interval per MCU row) is stated in
// ops/jpeg.py; ops/reference.py jpeg_encode_ref gives the same bytes.  Every table but the DCT
// matrix comes from the host in ``tab`` (ops.jpeg.device_tables), followed by the stream's header.
//
//   * jpeg_rows_kernel: one workgroup per (frame, MCU row), i.e. per restart interval.  In passes
//     of JP_CHUNK blocks: a thread per (block, column) transforms the columns, a thread per (block,
//     row) the rows and quantises into zigzag order in LDS; then a wave per block codes it, lane =
//     zigzag position: a ballot gives the non-zero mask, the run in front of a coefficient comes
//     from the mask below its lane, every lane forms its own ZRLs + code + value bits (at most 59)
//     and a wave scan (DPP) places them.  Block offsets are a scan over the pass; the bits are OR-ed into
//     the interval's bitstream in LDS.  A byte pass then counts the 0xFF bytes per 32-byte range,
//     scans, and writes the stuffed segment and its length to the workspace.
//   * jpeg_assemble_kernel: a wave per segment (and one for the header) sums the lengths in front
//     of its own, applies the overflow rule and copies to the final offset, then the RST / EOI
//     marker behind it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "aiko_api.h"

namespace aiko {

constexpr int JP_THREADS = 256;
constexpr int JP_WAVES = JP_THREADS / 64;
constexpr int JP_CHUNK = JP_THREADS / 8;              // blocks per pass: a thread per (block, column)
constexpr int JP_BPW = JP_CHUNK / JP_WAVES;           // blocks a wave codes per pass
constexpr int JP_MAX_W = 4096;
constexpr int JP_MAX_H = 65535;
constexpr int JP_MAX_BLOCKS = JP_MAX_W / 16 * 6;      // per MCU row: i420 (i444: 4096 / 8 * 3, the same)
constexpr int JP_MAX_SEG = 96 * 1024;                 // seg_cap: the interval's bitstream lives in LDS
// ``tab`` in 32-bit words (ops/jpeg.py): Huffman entries are code | length << 16, by symbol
constexpr int JP_T_AC = 0, JP_T_DC = 512, JP_T_Q = 544, JP_T_RCP = 672, JP_T_ZZ = 800, JP_TAB_INTS = 864;
static_assert(JP_CHUNK == 32 && JP_BPW == 8 && JP_MAX_BLOCKS == 1536, "the pass layout below");

// M[k][n] = round(8192 a_k cos((2n + 1) k pi / 16)): ops.jpeg.DCT_MATRIX (a test pins the two equal).
// y[k] = sum_n M[k][n] x[n], with M[k][7 - n] = (-1)^k M[k][n] folded first: integer sums are
// order-free, so these are the bits of the plain sum.
__device__ __forceinline__ void jp_dct8(const int (&x)[8], int (&y)[8]) {
  constexpr int JP_DCT[64] = {
      2896,  2896,  2896,  2896,  2896,  2896,  2896,  2896,
      4017,  3406,  2276,   799,  -799, -2276, -3406, -4017,
      3784,  1567, -1567, -3784, -3784, -1567,  1567,  3784,
      3406,  -799, -4017, -2276,  2276,  4017,   799, -3406,
      2896, -2896, -2896,  2896,  2896, -2896, -2896,  2896,
      2276, -4017,   799,  3406, -3406,  -799,  4017, -2276,
      1567, -3784,  3784, -1567, -1567,  3784, -3784,  1567,
       799, -2276,  3406, -4017,  4017, -3406,  2276,  -799};
  int s[4], d[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    s[n] = x[n] + x[7 - n];
    d[n] = x[n] - x[7 - n];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int acc = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) acc += JP_DCT[k * 8 + n] * ((k & 1) ? d[n] : s[n]);
    y[k] = acc;
  }
}

__device__ __forceinline__ int jp_wave_scan(int v, int lane) {     // inclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}

// The same scan of non-negative values in the data-parallel primitives: shifts by 1, 2, 4 and 8 within
// each row of 16 lanes, then row 0's total into row 1 and row 2's into row 3 (row_bcast:15), then
// the lower half's into the upper (row_bcast:31); a lane without a source adds 0.  Only bit offsets
// go through it: whatever they are, jp_emit stays inside the bitstream.
__device__ __forceinline__ int jp_wave_scan_dpp(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);     // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);     // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);     // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);     // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);     // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);     // row_bcast:31 into rows 2 and 3
  return v;
}

// OR the ``n`` (1..59) low bits of ``bits`` into the bitstream at bit ``pos``, MSB first; words at or
// past ``words`` are dropped (the interval has overflowed by then)
__device__ __forceinline__ void jp_emit(uint32_t* s_bits, int words, int pos, uint64_t bits, int n) {
  const uint64_t L = bits << (64 - n);
  const int wi = pos >> 5, sh = pos & 31;
  const uint64_t hi = L >> sh;
  const uint32_t w0 = (uint32_t)(hi >> 32), w1 = (uint32_t)hi;
  const uint32_t w2 = sh ? (uint32_t)((L << (64 - sh)) >> 32) : 0u;
  if (w0 && wi < words) atomicOr(&s_bits[wi], w0);
  if (w1 && wi + 1 < words) atomicOr(&s_bits[wi + 1], w1);
  if (w2 && wi + 2 < words) atomicOr(&s_bits[wi + 2], w2);
}

struct JpegRowArgs {
  const uint8_t* raw;           // [B, frame_bytes]
  const uint32_t* tab;          // JP_TAB_INTS words
  int* seglen;                  // [B, my]: the stuffed length, -1 past seg_cap
  uint8_t* seg;                 // [B, my, seg_cap]
  long frame_bytes;
  int H, W, is420, my, nblk;    // nblk: blocks per MCU row
  int seg_cap;
  int words, ranges;            // LDS: words = 8 * ranges >= ceil(seg_cap / 4) of bitstream
};

// Grid (my, B).  Dynamic LDS: the bitstream (``words``), then an 0xFF mask and an 0xFF prefix per
// 32-byte range (``ranges`` each).
__global__ __launch_bounds__(JP_THREADS) void jpeg_rows_kernel(const JpegRowArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t jp_lds[];
  __shared__ uint32_t s_tab[JP_TAB_INTS];
  __shared__ __attribute__((aligned(16))) int16_t s_t[JP_CHUNK * 64];      // [block][k][column]
  __shared__ int16_t s_coef[JP_CHUNK * 64];                                // [block][zigzag]
  __shared__ int16_t s_dc[JP_MAX_BLOCKS];                                  // the row's quantised DCs
  __shared__ int s_blen[JP_CHUNK];
  __shared__ int s_wsum[JP_WAVES];

  uint32_t* s_bits = jp_lds;
  uint32_t* s_mask = jp_lds + a.words;
  uint32_t* s_pref = s_mask + a.ranges;
  const int row = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, W = a.W;
  const int per = a.is420 ? 6 : 3;                    // blocks per MCU
  const uint8_t* frame = a.raw + (long)b * a.frame_bytes;

  for (int i = tid; i < JP_TAB_INTS; i += JP_THREADS) s_tab[i] = a.tab[i];
  for (int i = tid; i < a.words; i += JP_THREADS) s_bits[i] = 0u;
  __syncthreads();

  const uint32_t zrl2[2] = {s_tab[JP_T_AC + 0xF0], s_tab[JP_T_AC + 256 + 0xF0]};     // ZRL and EOB by table
  const uint32_t eob2[2] = {s_tab[JP_T_AC], s_tab[JP_T_AC + 256]};
  int bitpos = 0;                                     // bits coded so far: uniform
  for (int k0 = 0; k0 < a.nblk; k0 += JP_CHUNK) {
    // 1. columns: thread (block, column c)
    {
      const int blk = tid >> 3, c = tid & 7, k = k0 + blk;
      if (k < a.nblk) {
        const int mcu = k / per, sub = k - mcu * per;
        int pw, ph, bx, by;
        long base;
        if (a.is420 && sub < 4) {
          pw = W; ph = H; base = 0;
          bx = mcu * 16 + (sub & 1) * 8; by = row * 16 + (sub >> 1) * 8;
        } else if (a.is420) {
          pw = (W + 1) >> 1; ph = (H + 1) >> 1;
          base = (long)H * W + (long)(sub - 4) * pw * ph;
          bx = mcu * 8; by = row * 8;
        } else {
          pw = W; ph = H; base = (long)sub * H * W;
          bx = mcu * 8; by = row * 8;
        }
        const uint8_t* p = frame + base + min(bx + c, pw - 1);
        int x[8], y[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) x[n] = (int)p[(long)min(by + n, ph - 1) * pw] - 128;
        jp_dct8(x, y);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) s_t[blk * 64 + kk * 8 + c] = (int16_t)((y[kk] + 1024) >> 11);
      }
    }
    __syncthreads();
    // 2. rows and quantisation: thread (block, row kk)
    {
      const int blk = tid >> 3, kk = tid & 7, k = k0 + blk;
      if (k < a.nblk) {
        const int sub = k % per;
        const int tq = a.is420 ? (sub >= 4) : (sub != 0);
        int x[8], y[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) x[n] = s_t[blk * 64 + kk * 8 + n];
        jp_dct8(x, y);
#pragma unroll
        for (int l = 0; l < 8; ++l) {
          const int c = (y[l] + 16384) >> 15;
          const int z = (int)(s_tab[JP_T_ZZ + kk * 8 + l] & 63u);
          const uint32_t q = s_tab[JP_T_Q + tq * 64 + z], rcp = s_tab[JP_T_RCP + tq * 64 + z];
          const uint32_t num = (uint32_t)abs(c) + (q >> 1);             // < 2^16: the reciprocal is exact
          const int m = min((int)(q == 1u ? num : __umulhi(num, rcp)), 1023);
          const int v = c < 0 ? -m : m;
          s_coef[blk * 64 + z] = (int16_t)v;
          if (kk == 0 && l == 0) s_dc[k] = (int16_t)v;
        }
      }
    }
    __syncthreads();
    // 3. a wave per block, lane = zigzag position: every lane's bits and their place in the block
    uint64_t bits[JP_BPW];
    int nbit[JP_BPW], off[JP_BPW];
#pragma unroll
    for (int i = 0; i < JP_BPW; ++i) {
      const int blk = i * JP_WAVES + wave, k = k0 + blk;
      bits[i] = 0;
      nbit[i] = 0;
      off[i] = 0;
      if (k >= a.nblk) {                              // uniform in the wave
        if (lane == 0) s_blen[blk] = 0;
        continue;
      }
      const int sub = k % per;
      const int tc = a.is420 ? (sub >= 4) : (sub != 0);
      int v = s_coef[blk * 64 + lane];
      if (lane == 0) {                                // the DC difference to the component's last block
        int prev;
        if (a.is420)
          prev = sub >= 4 ? k - 6 : (sub == 0 ? k - 3 : k - 1);
        else
          prev = k - 3;
        v -= prev >= 0 ? (int)s_dc[prev] : 0;
      }
      const int mag = abs(v);
      const int size = 32 - __clz(mag);               // 0 for 0; at most 11
      const uint32_t vb = (uint32_t)(v < 0 ? v + (1 << size) - 1 : v) & ((1u << size) - 1u);
      const uint64_t nz = __ballot(lane > 0 && v != 0);
      uint64_t w = 0;
      int n = 0;
      if (lane == 0) {
        const uint32_t e = s_tab[JP_T_DC + tc * 16 + size];
        w = ((uint64_t)(e & 0xffffu) << size) | vb;
        n = (int)((e >> 16) & 31u) + size;
      } else if (v != 0) {
        const uint64_t below = (nz & ((1ull << lane) - 1ull)) | 1ull;    // bit 0: the DC ends every run
        const int run = lane - (63 - __clzll((long long)below)) - 1;
        const uint32_t e = s_tab[JP_T_AC + tc * 256 + (((run & 15) << 4) | size)];
        const uint32_t zrl = tc ? zrl2[1] : zrl2[0];
        const int zl = (int)((zrl >> 16) & 31u), el = (int)((e >> 16) & 31u);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < (run >> 4)) {
            w = (w << zl) | (zrl & 0xffffu);
            n += zl;
          }
        w = (((w << el) | (e & 0xffffu)) << size) | vb;
        n += el + size;                               // at most 3 * 11 + 16 + 10 = 59
      } else if (lane == 63) {                        // coefficient 63 is zero: EOB
        const uint32_t e = tc ? eob2[1] : eob2[0];
        w = e & 0xffffu;
        n = (int)((e >> 16) & 31u);
      }
      const int inc = jp_wave_scan_dpp(n);
      bits[i] = w;
      nbit[i] = n;
      off[i] = inc - n;
      if (lane == 63) s_blen[blk] = inc;
    }
    __syncthreads();
    // 4. the blocks' places in the interval, then the bits
    {
      const int bl = lane < JP_CHUNK ? s_blen[lane] : 0;
      const int inc = jp_wave_scan_dpp(bl);
      const int excl = inc - bl;
#pragma unroll
      for (int i = 0; i < JP_BPW; ++i) {
        const int at = bitpos + __shfl(excl, i * JP_WAVES + wave) + off[i];
        if (nbit[i] > 0) jp_emit(s_bits, a.words, at, bits[i], nbit[i]);
      }
      bitpos += __shfl(inc, 63);
    }
    // s_t, s_coef and s_blen are next written behind the barriers of the next pass
  }
  __syncthreads();
  if (tid == 0 && (bitpos & 7)) {                     // pad the last byte with 1-bits
    const int n = 8 - (bitpos & 7);
    jp_emit(s_bits, a.words, bitpos, (1ull << n) - 1ull, n);
  }
  __syncthreads();

  const long slot = (long)b * a.my + row;
  const int nb = (bitpos + 7) >> 3;                   // bytes before stuffing
  if (nb > a.seg_cap) {                               // uniform
    if (tid == 0) a.seglen[slot] = -1;
    return;
  }
  // the 0xFF bytes of every 32-byte range (8 words; byte j of the stream is bits 31 - 8 (j & 3) ...
  // of word j >> 2), a thread's ranges consecutive; bytes at and past nb are zero
  const int nr = (nb + 31) >> 5;                      // <= ranges
  const int rp = (nr + JP_THREADS - 1) / JP_THREADS;
  const int r0 = min(tid * rp, nr), r1 = min(r0 + rp, nr);
  int cnt = 0;
  for (int r = r0; r < r1; ++r) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t w = s_bits[r * 8 + j];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (((w >> (24 - 8 * q)) & 0xffu) == 0xffu) m |= 1u << (j * 4 + q);
    }
    s_mask[r] = m;
    s_pref[r] = (uint32_t)cnt;
    cnt += __popc(m);
  }
  const int inc = jp_wave_scan(cnt, lane);
  if (lane == 63) s_wsum[wave] = inc;
  __syncthreads();
  int before = inc - cnt, total = 0;
#pragma unroll
  for (int w = 0; w < JP_WAVES; ++w) {
    if (w < wave) before += s_wsum[w];
    total += s_wsum[w];
  }
  for (int r = r0; r < r1; ++r) s_pref[r] += (uint32_t)before;
  const int stuffed = nb + total;
  if (tid == 0) a.seglen[slot] = stuffed > a.seg_cap ? -1 : stuffed;
  if (stuffed > a.seg_cap) return;                    // uniform
  __syncthreads();
  uint8_t* out = a.seg + slot * a.seg_cap;
  for (int i = tid; i < nb; i += JP_THREADS) {
    const uint32_t byte = (s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu;
    const int r = i >> 5;
    const int j = i + (int)s_pref[r] + __popc(s_mask[r] & ((1u << (i & 31)) - 1u));   // < stuffed
    out[j] = (uint8_t)byte;
    if (byte == 0xffu) out[j + 1] = 0;
  }
}

struct JpegAssembleArgs {
  const uint8_t* header;
  const int* seglen;            // [B, my]
  const uint8_t* seg;           // [B, my, seg_cap]
  uint8_t* stream;              // [B, cap]
  int* nbytes;                  // [B]
  int header_len, my, seg_cap, cap;
};

// ``n`` bytes by one wave: bytes up to dst's first dword boundary, aligned dword stores (the source
// read as it lies), the bytes left over
__device__ __forceinline__ void jp_wave_copy(uint8_t* dst, const uint8_t* src, int n, int lane) {
  const int head = min(n, (int)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
  if (lane < head) dst[lane] = src[lane];
  const int nw = (n - head) >> 2;
  for (int i = lane; i < nw; i += 64) {
    uint32_t v;
    memcpy(&v, src + head + 4 * i, 4);
    *reinterpret_cast<uint32_t*>(dst + head + 4 * i) = v;
  }
  const int t0 = head + 4 * nw;
  if (lane < n - t0) dst[t0 + lane] = src[t0 + lane];
}

// Grid (ceil((my + 1) / JP_WAVES), B); wave job 0 of a frame is the header and ``nbytes``, job j the
// segment of MCU row j - 1 and the marker behind it.  Every wave sums all the frame's lengths
// itself: no LDS, no barrier.  An overflowed frame gets its -1 and nothing else.
__global__ __launch_bounds__(JP_THREADS) void jpeg_assemble_kernel(const JpegAssembleArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int job = blockIdx.x * JP_WAVES + (threadIdx.x >> 6);
  if (job > a.my) return;
  const int r = job - 1;
  const int* len = a.seglen + (long)b * a.my;
  long tot = 0, pre = 0;
  int bad = 0;
  for (int j = lane; j < a.my; j += 64) {
    const int l = len[j];
    bad |= l < 0;
    tot += l;
    if (j < r) pre += l;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    tot += __shfl_xor(tot, d);
    pre += __shfl_xor(pre, d);
    bad |= __shfl_xor(bad, d);
  }
  const long total = (long)a.header_len + tot + 2L * a.my;       // my - 1 RSTs and the EOI
  const bool overflow = bad || total > (long)a.cap;
  uint8_t* out = a.stream + (long)b * a.cap;
  if (job == 0) {
    if (lane == 0) a.nbytes[b] = overflow ? -1 : (int)total;
    if (!overflow) jp_wave_copy(out, a.header, a.header_len, lane);
    return;
  }
  if (overflow) return;
  const int n = len[r];
  const long at = (long)a.header_len + pre + 2L * r;
  jp_wave_copy(out + at, a.seg + ((long)b * a.my + r) * a.seg_cap, n, lane);
  if (lane < 2) out[at + n + lane] = lane == 0 ? 0xff : (uint8_t)(r < a.my - 1 ? 0xd0 + (r & 7) : 0xd9);
}

}  // namespace aiko

namespace {

// MCU rows of a frame, or 0 for a geometry the launches do not cover
int jpeg_rows(int B, int H, int W, int fmt, int seg_cap, const void* workspace) {
  if ((fmt != 1 && fmt != 2) || B < 1 || B > 65535 || H < 1 || H > aiko::JP_MAX_H || W < 1 || W > aiko::JP_MAX_W ||
      seg_cap < 1 || seg_cap > aiko::JP_MAX_SEG || reinterpret_cast<uintptr_t>(workspace) % 4)
    return 0;
  const int mcu = fmt == 1 ? 16 : 8;
  return (H + mcu - 1) / mcu;
}

}  // namespace

// The three entry points return -1 for a configuration the launches do not cover.  fmt 1: i420, 2:
// i444 (the codes of ops.yuv.FORMATS); my = ceil(H / MCU height); tables: ops.jpeg.device_tables,
// 4-byte aligned, JP_TAB_INTS words and then header_len bytes of header; workspace: 4-byte aligned,
// an int32 [B, my] of segment lengths and then uint8 [B, my, seg_cap].
// The row pass: raw uint8 [B, frame_bytes(fmt, H, W)] -> the workspace.
extern "C" int aiko_jpeg_rows(const void* raw, const void* tables, void* workspace, int B, int H, int W, int fmt,
                              int seg_cap, hipStream_t strm) {
  using namespace aiko;
  const int my = jpeg_rows(B, H, W, fmt, seg_cap, workspace);
  if (!my || reinterpret_cast<uintptr_t>(tables) % 4) return -1;
  const int is420 = fmt == 1;
  const int mcu = is420 ? 16 : 8;
  const int mx = (W + mcu - 1) / mcu;
  const long ch = (H + 1) / 2, cw = (W + 1) / 2;
  JpegRowArgs r;
  r.raw = static_cast<const uint8_t*>(raw);
  r.tab = static_cast<const uint32_t*>(tables);
  r.seglen = static_cast<int*>(workspace);
  r.seg = static_cast<uint8_t*>(workspace) + 4L * B * my;
  r.frame_bytes = is420 ? (long)H * W + 2 * ch * cw : 3L * H * W;
  r.H = H; r.W = W; r.is420 = is420; r.my = my;
  r.nblk = mx * (is420 ? 6 : 3);
  r.seg_cap = seg_cap;
  r.ranges = (seg_cap + 31) / 32;
  r.words = 8 * r.ranges;
  const size_t lds = 4ul * (r.words + 2 * r.ranges);
  if (lds > 64 * 1024) {                              // per device and function: set where it is needed
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&jpeg_rows_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  jpeg_rows_kernel<<<dim3((unsigned)my, (unsigned)B), JP_THREADS, lds, strm>>>(r);
  return (int)hipGetLastError();
}

// The assembly: the workspace and the header -> stream uint8 [B, cap], nbytes int32 [B].
extern "C" int aiko_jpeg_assemble(const void* tables, int header_len, const void* workspace, void* stream, int* nbytes,
                                  int B, int H, int W, int fmt, long cap, int seg_cap, hipStream_t strm) {
  using namespace aiko;
  const int my = jpeg_rows(B, H, W, fmt, seg_cap, workspace);
  if (!my || header_len < 1 || cap < 1 || cap > INT32_MAX) return -1;
  JpegAssembleArgs s;
  s.header = static_cast<const uint8_t*>(tables) + 4 * JP_TAB_INTS;
  s.seglen = static_cast<const int*>(workspace);
  s.seg = static_cast<const uint8_t*>(workspace) + 4L * B * my;
  s.stream = static_cast<uint8_t*>(stream);
  s.nbytes = nbytes;
  s.header_len = header_len; s.my = my; s.seg_cap = seg_cap; s.cap = (int)cap;
  jpeg_assemble_kernel<<<dim3((unsigned)((my + 1 + JP_WAVES - 1) / JP_WAVES), (unsigned)B), JP_THREADS, 0, strm>>>(s);
  return (int)hipGetLastError();
}

// One encode: both passes on ``strm``, nothing launched unless both are covered.
extern "C" int aiko_jpeg_encode(const void* raw, const void* tables, int header_len, void* workspace, void* stream,
                                int* nbytes, int B, int H, int W, int fmt, long cap, int seg_cap,
                                hipStream_t strm) {
  if (header_len < 1 || cap < 1 || cap > INT32_MAX) return -1;
  const int rc = aiko_jpeg_rows(raw, tables, workspace, B, H, W, fmt, seg_cap, strm);
  return rc ? rc : aiko_jpeg_assemble(tables, header_len, workspace, stream, nbytes, B, H, W, fmt, cap, seg_cap, strm);
}
