// The serial part of baseline JPEG decoding (the rule: ops/jpeg_decode.py): a bit reader bounded by
// its restart interval and the Huffman decoder of one interval's blocks.  One text for two compilers:
// under hipcc the functions are __host__ __device__ and a lane of jpeg_entropy_kernel runs them; under
// a host compiler they are plain inline functions (no HIP header is included), which a stand-alone
// program runs under the sanitizers (tests/native/jpeg_decode_core_main.cpp).
//
// Bounds: every read of ``data`` is at an index in [start, end) of the interval; every loop is counted
// (MCUs of the interval, blocks of an MCU, at most 63 AC symbols of a block, 16 lengths of a code, 8
// bytes of a refill); table indices are masked to the tables' sizes, so a descriptor of any content
// reads inside itself; coefficient stores go to the 64 slots of the block being decoded.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JD_FN __host__ __device__ __forceinline__
#else
#define JD_FN static inline
#endif

namespace aiko {

// The descriptor of one header (ops.jpeg_decode.plan_bytes), in bytes / 32-bit words
constexpr int JD_PLAN_BYTES = 1744;
constexpr int JD_PLAN_WORDS = JD_PLAN_BYTES / 4;
constexpr int JD_P_SCAN = 0, JD_P_DRI = 4, JD_P_SEL = 8, JD_P_Q = 16, JD_P_HUFF = 208, JD_HUFF_BYTES = 384;
// status bits
constexpr int JD_E_MARKER = 1, JD_E_CODE = 2, JD_E_END = 4, JD_E_RUN = 8, JD_E_STUFF = 16;

// blocks per MCU of the raw formats (the codes of ops.yuv.FORMATS): 1 i420, 2 i444, 3 yuyv (4:2:2)
JD_FN int jd_blocks_per_mcu(int fmt) { return fmt == 1 ? 6 : (fmt == 2 ? 3 : 4); }
// the component of block ``sub`` of an MCU
JD_FN int jd_component(int fmt, int sub) {
  const int luma = fmt == 1 ? 4 : (fmt == 2 ? 1 : 2);
  return sub < luma ? 0 : sub - luma + 1;
}

// MSB-first bits of data[start, end) with FF 00 read as FF.  ``acc`` holds ``nbits`` bits, its low
// ``fake`` ones zeros that stand for what lies behind the readable bytes: the interval's end
// (fake_err = JD_E_END) or an FF that no 00 follows (JD_E_STUFF).  Such bits are an error only once
// they are consumed.
struct JdBits {
  const uint8_t* data;
  int pos, end;
  uint64_t acc;
  int nbits, fake, fake_err;
};

JD_FN void jd_open(JdBits& r, const uint8_t* data, int start, int end) {
  r.data = data;
  r.pos = start;
  r.end = end;
  r.acc = 0;
  r.nbits = 0;
  r.fake = 0;
  r.fake_err = 0;
}

// at least 57 bits in acc
JD_FN void jd_fill(JdBits& r) {
  for (int i = 0; i < 8 && r.nbits <= 56; ++i) {
    uint32_t byte = 0;
    if (r.fake_err == 0) {
      if (r.pos >= r.end) {
        r.fake_err = JD_E_END;
      } else {
        byte = r.data[r.pos];
        if (byte != 0xffu) {
          r.pos += 1;
        } else if (r.pos + 1 < r.end && r.data[r.pos + 1] == 0) {
          r.pos += 2;
        } else {
          r.fake_err = JD_E_STUFF;
          byte = 0;
        }
      }
    }
    if (r.fake_err) r.fake += 8;
    r.acc = (r.acc << 8) | byte;
    r.nbits += 8;
  }
}

// the next ``n`` (0..16) bits without consuming them; jd_fill first
JD_FN uint32_t jd_peek(const JdBits& r, int n) {
  return (uint32_t)(r.acc >> (r.nbits - n)) & ((1u << n) - 1u);
}

// consume ``n`` peeked bits: 0, or the error of a bit that is not there
JD_FN int jd_skip(JdBits& r, int n) {
  r.nbits -= n;
  return r.nbits < r.fake ? r.fake_err : 0;
}

// One Huffman symbol by the table at ``tab`` (16 maxcode words, 16 valoff words, 256 symbol bytes):
// 0..255, or -error
JD_FN int jd_symbol(JdBits& r, const uint32_t* tab) {
  jd_fill(r);
  const uint32_t w = jd_peek(r, 16);
  for (int l = 1; l <= 16; ++l) {
    const int code = (int)(w >> (16 - l));
    if (code <= (int)tab[l - 1]) {
      const int e = jd_skip(r, l);
      if (e) return -e;
      const uint32_t idx = (uint32_t)(code + (int)tab[16 + l - 1]) & 255u;
      return (int)((tab[32 + (idx >> 2)] >> (8 * (idx & 3u))) & 255u);
    }
  }
  return r.nbits - r.fake < 16 ? -r.fake_err : -JD_E_CODE;
}

// ``s`` (1..15) value bits, extended; the error through ``err``
JD_FN int jd_value(JdBits& r, int s, int& err) {
  jd_fill(r);
  const int v = (int)jd_peek(r, s);
  err = jd_skip(r, s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// The blocks of the MCUs [mcu0, mcu1) of one frame, which lie in data[start, end): int16 coefficients
// in zigzag order to coef[(mcu * per + sub) * 64 + z], zeros for what a block does not code.
// ``plan``: the descriptor's words (JD_PLAN_WORDS of them, 4-byte aligned).  Returns the status bits.
JD_FN int jd_interval(const uint8_t* data, int start, int end, const uint32_t* plan, int fmt, int mcu0, int mcu1,
                      int16_t* coef) {
  JdBits r;
  jd_open(r, data, start, end);
  const int per = jd_blocks_per_mcu(fmt);
  const uint32_t sel = plan[JD_P_SEL / 4], sel2 = plan[JD_P_SEL / 4 + 1];
  int pred0 = 0, pred1 = 0, pred2 = 0;
  for (int mcu = mcu0; mcu < mcu1; ++mcu) {
    for (int sub = 0; sub < per; ++sub) {
      const int comp = jd_component(fmt, sub);
      // selector bytes: dc 8, 9, 10; ac 11, 12, 13
      const uint32_t dsel = (sel >> (8 * comp)) & 1u;
      const uint32_t asel = (comp == 0 ? sel >> 24 : sel2 >> (8 * (comp - 1))) & 1u;
      const uint32_t* dct = plan + (JD_P_HUFF + (int)dsel * JD_HUFF_BYTES) / 4;
      const uint32_t* act = plan + (JD_P_HUFF + (2 + (int)asel) * JD_HUFF_BYTES) / 4;
      // ``coef`` is 16-byte aligned and a block is 128 bytes: wide stores
      int16_t* out = static_cast<int16_t*>(__builtin_assume_aligned(coef + ((long)mcu * per + sub) * 64, 16));
      __builtin_memset(out, 0, 128);
      int err = 0;
      const int t = jd_symbol(r, dct);
      if (t < 0) return -t;
      const int s = t & 15;
      int diff = 0;
      if (s) {
        diff = jd_value(r, s, err);
        if (err) return err;
      }
      int p = (comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2)) + diff;
      p = p < -32768 ? -32768 : (p > 32767 ? 32767 : p);
      if (comp == 0) pred0 = p; else if (comp == 1) pred1 = p; else pred2 = p;
      out[0] = (int16_t)p;
      int k = 1;
      for (int n = 0; n < 63 && k < 64; ++n) {
        const int rs = jd_symbol(r, act);
        if (rs < 0) return -rs;
        const int run = rs >> 4, size = rs & 15;
        if (size == 0) {
          if (run != 15) break;                             // EOB
          if (k + 16 > 64) return JD_E_RUN;
          k += 16;
          continue;
        }
        k += run;
        if (k > 63) return JD_E_RUN;
        const int v = jd_value(r, size, err);
        if (err) return err;
        out[k] = (int16_t)v;
        k += 1;
      }
    }
  }
  return 0;
}

// The marker scan of one frame, serially (the kernel's is parallel): the start of every interval to
// starts[0 .. intervals), the frame's interval count to *count; returns 0 or JD_E_MARKER.
// ``nbytes`` beyond ``cap`` or below 1, a scan offset outside the stream, more intervals than
// ``max_intervals``, no EOI at nbytes - 2, a wrong number or order of RST markers: JD_E_MARKER.
JD_FN int jd_scan_serial(const uint8_t* data, int nbytes, long cap, const uint32_t* plan, int mcus, int max_intervals,
                         int* starts, int* count) {
  const int scan = (int)plan[JD_P_SCAN / 4], dri = (int)plan[JD_P_DRI / 4];
  *count = 0;
  if (nbytes < 1 || nbytes > cap || scan < 2 || scan > nbytes - 2 || dri < 0) return JD_E_MARKER;
  const int n = dri > 0 ? (mcus + dri - 1) / dri : 1;
  if (n > max_intervals) return JD_E_MARKER;
  *count = n;
  int bad = !(data[nbytes - 2] == 0xff && data[nbytes - 1] == 0xd9);
  int found = 0;
  starts[0] = scan;
  for (int i = scan; i + 1 < nbytes - 2; ++i) {
    if (data[i] == 0xff && (data[i + 1] & 0xf8) == 0xd0) {
      if (found < n - 1) {
        starts[found + 1] = i + 2;
        bad |= (data[i + 1] & 7) != (found & 7);
      }
      found += 1;
    }
  }
  return bad || found != n - 1 ? JD_E_MARKER : 0;
}

}  // namespace aiko
