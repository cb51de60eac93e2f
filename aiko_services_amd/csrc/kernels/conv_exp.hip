// A ResNet bottleneck's 3x3 conv fused with its 1x1 expansion, identity residual and ReLU:
//   y = relu(W3 . relu(conv3x3(t1, W2) + b2) + b3 + x)      (256 -> 256 -> N channels)
//
// Phase 1 is conv_wide.hip's 256 x 256 tile (transposed product, 2-slot LDS-DMA ring of 64-deep
// K blocks with XOR-swizzled 128-B rows, scalar tap cursor, counted vmcnt + raw s_barrier).  The
// tile covers all 256 mid channels, so when its K loop ends the workgroup owns a complete
// 256-pixel slice of t2.  Rounded to bf16 (what the unfused path writes to HBM) that slice is
// 128 KB — exactly the dead ring — and is written there as four [256 px][64 ch] blocks with the
// swizzle the pixel-side fragment reads expect: after v_permlane16_swap a lane holds 8
// consecutive channels of one pixel, one ds_write_b128.
//
// Phase 2 walks the N output channels in chunks of 128 (2 x 4 waves of 128 pixels x 32
// channels, 64 accumulator VGPRs).  The pixel operand comes from the resident t2 blocks, read
// into a rolling 8-fragment window.  The weight operand never touches LDS: W3 is packed once on
// the host in MFMA fragment order (ops.conv.exp_weight: [N / 16][K / 32][64 lanes][8]), so a
// wave's fragment is one contiguous 1 KB buffer load, held in a rolling window of four 32-deep
// K slices that is refilled, as soon as the MFMAs have consumed a slice, with the slice four
// ahead (the next chunk's from slice 4 on).  Phase 2 therefore has no barrier at all: the eight
// waves drift apart and one wave's residual loads and stores run under the others' MFMAs.  The
// residual is double-buffered in registers and loaded TWO chunks ahead, right after the epilogue
// that frees its buffer (one chunk ahead measured 2 % slower).  Loads and
// stores are buffer ops that are always issued: pixel rows >= M fall outside the res / y
// buffer resources, whose size is the tensor's, and the chunks past the last get an
// out-of-range offset, so there is no divergent control flow around them and nothing is
// written for rows >= M.
//
// Register budget: one 512-thread workgroup per CU leaves 256 VGPRs per wave and phase 1 uses
// all of them, so everything phase 2 needs is derived after the K loop from a lane id that the
// compiler cannot trace back (else it keeps it all alive through the K loop, in scratch).
//
// W3 staging and grid alternatives, measured: profiles/conv3x3_exp.md.
#include <type_traits>

#include "conv_common.h"
#include "conv_wide_stage.h"
#include "aiko_api.h"

namespace aiko {

typedef __attribute__((ext_vector_type(2))) short i16x2;

// ReLU of a packed bf16 pair: negative values (sign bit set, -0 included) are the negative int16s
__device__ __forceinline__ uint32_t relu_bf16x2(uint32_t v) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2, v), i16x2{0, 0}));
}

struct ConvExpParams {
  ConvParams c;        // phase 1: x = t1, w = W2 [256][9 * 256], bias = b2; res / y / ldr / ldy of phase 2
  const bf16_t* w3;    // fragment image of W3 [N][256]
  const float* b3;     // [N]
  int N;               // output channels (multiple of 128)
};

__global__ __launch_bounds__(512, 1) void conv3x3_exp_kernel(ConvExpParams q) {
  const ConvParams& p = q.c;
  constexpr int BM = 256, BN = 256, BK = 64, WGN = 4, NW = 8, NS = 2;
  constexpr int WM = 128, WN = 64, MI = 8, NI = 4, NP = 2;
  constexpr int RPW = 8, RPI = 64, APT = 4, BPT = 4;
  constexpr int STAGE_ELEMS = (BM + BN) * BK;
  constexpr int T2_BLOCK = BM * 64;                 // one [256 px][64 ch] block of the t2 slice
  static_assert(NS * STAGE_ELEMS == 4 * T2_BLOCK, "the t2 slice fills the ring exactly");
  __shared__ __attribute__((aligned(16))) bf16_t ring[NS * STAGE_ELEMS];

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / WGN, wc = wave % WGN;
  const int ntiles = (p.M + BM - 1) / BM;
  const int G = gridDim.x;
  const int lid = xcd_remap(blockIdx.x, G);

  const __amdgpu_buffer_rsrc_t rx = wide_rsrc(p.x);
  const __amdgpu_buffer_rsrc_t rw = wide_rsrc(p.w);
  const __amdgpu_buffer_rsrc_t rw3 = wide_rsrc(q.w3);
  // res / y: num_records is the tensor's exact size, so pixel rows >= M (the last tile's tail)
  // are out of range on their own: their loads return zero and their stores are dropped
  const int io_bytes = p.M * q.N * 2;
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.res), (short)0, io_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.y, (short)0, io_bytes, 0x00020000);

  const int nkb = p.K / BK;
  const int nch = q.N / 128;

  for (int tile = lid; tile < ntiles; tile += G) {
    const int m0 = tile * BM;
    // lane geometry from a lane id counted afresh (v_mbcnt) and opaque, per tile and again for
    // phase 2: the K loop has no registers to spare for values kept alive around it
    uint32_t lz = 0u;
    asm volatile("" : "+v"(lz));
    const int lane1 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, lz));
    const int lrow = wave * RPW + (lane1 >> 3);
    const int lp = (lane1 & 7) ^ (lane1 >> 3);          // source-side swizzle
    const int HoWo = p.Ho * p.Wo;
    uint32_t b_off[BPT];
#pragma unroll
    for (int i = 0; i < BPT; ++i) b_off[i] = (uint32_t)(((lrow + RPI * i) * p.K + lp * 8) * 2);

    const int fr = lane1 & 15, fq = lane1 >> 4;
    const int coff = ((fq & 1) << 4) | ((fq >> 1) << 3);
    const int sw = fr & 7;

    // ---------------- phase 1: t2 tile = conv3x3(t1), as conv_wide<256, 256, 2, 4, 2> ----------
    int a_base[APT];
    uint32_t a_mask[APT], a_off[APT];
#pragma unroll
    for (int i = 0; i < APT; ++i) {
      const int m = m0 + lrow + RPI * i;
      a_mask[i] = 0u;
      a_base[i] = 0;
      a_off[i] = kWideOOB;
      if (m < p.M) {
        const int img = fdiv(m, p.mHoWo, p.lHoWo);
        const int rem = m - img * HoWo;
        const int oh = fdiv(rem, p.mWo, p.lWo);
        const int ow = rem - oh * p.Wo;
        const int ih0 = oh * p.stride - p.pad, iw0 = ow * p.stride - p.pad;
        a_base[i] = (((img * p.H + ih0) * p.W + iw0) * p.C + lp * 8) * 2;
        const int r_lo = max(0, -ih0), r_hi = min(p.R, p.H - ih0);
        const int s_lo = max(0, -iw0), s_hi = min(p.S, p.W - iw0);
        const uint32_t mr = r_hi > r_lo ? ((1u << r_hi) - 1u) & ~((1u << r_lo) - 1u) : 0u;
        const uint32_t ms = s_hi > s_lo ? ((1u << s_hi) - 1u) & ~((1u << s_lo) - 1u) : 0u;
        a_mask[i] = mr | (ms << 16);
      }
    }
    // b2 for the hand-over: in flight under the first K blocks (older than block 0's DMAs)
    float e_bias[NP][8];
#pragma unroll
    for (int h = 0; h < NP; ++h) {
      const int n = wc * WN + h * 32 + coff;
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.bias + n);
      const f32x4 b1 = *reinterpret_cast<const f32x4*>(p.bias + n + 4);
      e_bias[h][0] = b0[0]; e_bias[h][1] = b0[1]; e_bias[h][2] = b0[2]; e_bias[h][3] = b0[3];
      e_bias[h][4] = b1[0]; e_bias[h][5] = b1[1]; e_bias[h][6] = b1[2]; e_bias[h][7] = b1[3];
    }

    int cur_tap = -1, iss_tap = 0, iss_c = 0, iss_r = 0, iss_s = 0;
    auto issue = [&](int kb, auto slot_tag) {
      constexpr int SLOT = decltype(slot_tag)::value;
      bf16_t* Xs = ring + SLOT * STAGE_ELEMS;
      bf16_t* Ws = Xs + BM * BK;
      const uint32_t sb = (uint32_t)(kb * BK * 2);
#pragma unroll
      for (int i = 0; i < BPT; ++i) wide_dma16(rw, b_off[i], sb, Ws + (i * RPI + wave * RPW) * BK);
      if (iss_tap != cur_tap) {
        cur_tap = iss_tap;
        const int tap_off = ((iss_r * p.W + iss_s) * p.C) * 2;
        const uint32_t bit = (1u << iss_r) | (1u << (iss_s + 16));
#pragma unroll
        for (int i = 0; i < APT; ++i)
          a_off[i] = (a_mask[i] & bit) == bit ? (uint32_t)(a_base[i] + tap_off) : kWideOOB;
      }
      const uint32_t soff = (uint32_t)(iss_c * 2);
#pragma unroll
      for (int i = 0; i < APT; ++i) wide_dma16(rx, a_off[i], soff, Xs + (i * RPI + wave * RPW) * BK);
      iss_c += BK;
      if (iss_c >= p.Cc) {
        iss_c = 0;
        ++iss_tap;
        if (++iss_s == p.S) {
          iss_s = 0;
          ++iss_r;
        }
      }
    };

    f32x4 acc[NI][MI];
    float zero = 0.f;                               // opaque, or the zero tile is hoisted out of the
    asm volatile("" : "+v"(zero));                  // tile loop and kept in registers across it
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int i = 0; i < MI; ++i) acc[j][i] = f32x4{zero, zero, zero, zero};

    int w_rd[NI], x_rd[MI];
#pragma unroll
    for (int j = 0; j < NI; ++j) w_rd[j] = BM * BK + (wc * WN + j * 16 + fr) * BK;
#pragma unroll
    for (int i = 0; i < MI; ++i) x_rd[i] = (wr * WM + i * 16 + fr) * BK;

    auto compute = [&](auto slot_tag) {
      constexpr int SLOT = decltype(slot_tag)::value;
      const bf16_t* St = ring + SLOT * STAGE_ELEMS;
#pragma unroll
      for (int kk = 0; kk < BK / 32; ++kk) {
        const int pc = ((fq + 4 * kk) ^ sw) << 3;
        bf16x8 wf[NI], xf[MI];
#pragma unroll
        for (int j = 0; j < NI; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(St + w_rd[j] + pc);
#pragma unroll
        for (int i = 0; i < MI; ++i) xf[i] = *reinterpret_cast<const bf16x8*>(St + x_rd[i] + pc);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[i], acc[j][i], 0, 0, 0);
      }
    };

    auto step = [&](int kb, auto slot_tag) {
      constexpr int SLOT = decltype(slot_tag)::value;
      wide_vm_barrier<0>();                         // block kb has landed; the other slot is free
      if (kb + 1 < nkb) issue(kb + 1, std::integral_constant<int, 1 - SLOT>{});
      compute(slot_tag);
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    issue(0, S0{});
    {
      int kb = 0;
      for (; kb + 2 <= nkb; kb += 2) {
        step(kb, S0{});
        step(kb + 1, S1{});
      }
      if (kb < nkb) step(kb, S0{});
    }

    // ---------------- hand-over: bias, ReLU, bf16, swap, one ds_write_b128 per 8 channels -------
    uint32_t lz2 = 0u;
    asm volatile("" : "+v"(lz2));
    const int lane2 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, lz2));
    const int fr2 = lane2 & 15, fq2 = lane2 >> 4;
    const int coff2 = ((fq2 & 1) << 4) | ((fq2 >> 1) << 3);
    const int sw2 = fr2 & 7;
    const int x_r0 = (wr * WM + fr2) * 64;
    __syncthreads();                               // every wave has read its last K block
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
      for (int h = 0; h < NP; ++h) {
        f32x4 lo = acc[2 * h][i], hi = acc[2 * h + 1][i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(lo[e]), __float_as_uint(hi[e]), false, false);
          lo[e] = __uint_as_float(s[0]);
          hi[e] = __uint_as_float(s[1]);
        }
        u32x4 o;
        o[0] = pack2(fmaxf(lo[0] + e_bias[h][0], 0.f), fmaxf(lo[1] + e_bias[h][1], 0.f));
        o[1] = pack2(fmaxf(lo[2] + e_bias[h][2], 0.f), fmaxf(lo[3] + e_bias[h][3], 0.f));
        o[2] = pack2(fmaxf(hi[0] + e_bias[h][4], 0.f), fmaxf(hi[1] + e_bias[h][5], 0.f));
        o[3] = pack2(fmaxf(hi[2] + e_bias[h][6], 0.f), fmaxf(hi[3] + e_bias[h][7], 0.f));
        // t2 channel wc * 64 + h * 32 + coff2: block wc, logical 16-B piece h * 4 + coff2 / 8
        const int piece = (h * 4 + (coff2 >> 3)) ^ sw2;
        *reinterpret_cast<u32x4*>(ring + wc * T2_BLOCK + (x_r0 + i * 16 * 64) + (piece << 3)) = o;
      }
    }

    // ---------------- phase 2: y chunk = relu(W3 chunk . t2 + b3 + x), 128 channels at a time ---
    // per-lane byte offsets: the first of the lane's 8 pixel rows of res / y (16 rows apart), W3
    // fragments
    const uint32_t row0 = (uint32_t)(((m0 + wr * WM + fr2) * q.N + wc * 32 + coff2) * 2);
    const uint32_t row_step = (uint32_t)(16 * q.N * 2);
    const uint32_t w_off = (uint32_t)(wc * 2 * 8 * 1024 + lane2 * 16);
    bf16x8 wreg[4][2];                              // window of 4 32-deep K slices x 2 channel blocks
    u32x4 e_res[2][MI];                             // residual of this chunk and the next
    f32x2 e_b3[4];
    // K slice ks of chunk c (chunks past the last: out of range, nothing is fetched)
    auto load_w = [&](int c, int ks) __attribute__((always_inline)) {
      const uint32_t base = c < nch ? w_off : kWideOOB;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        wreg[ks & 3][j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
            rw3, base, (uint32_t)c * 65536u + (uint32_t)((j * 8 + ks) * 1024), 0));   // scalar offset: one address register
    };
    auto load_res = [&](int c, auto par_tag) __attribute__((always_inline)) {
      constexpr int P = decltype(par_tag)::value;
      const uint32_t cb = (uint32_t)c * 256u;
      const uint32_t base = c < nch ? row0 : kWideOOB;
      uint32_t rs = row_step;                       // opaque: the 8 row offsets are recomputed at
      asm volatile("" : "+s"(rs));                  // each use, not kept in 8 registers
#pragma unroll
      for (int i = 0; i < MI; ++i)
        e_res[P][i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
            rr, base + rs * i, cb, 0));
    };
    // the chunk's 8 bias values: from L2, loaded at the head of the chunk's own K loop
    auto load_b3 = [&](int c) __attribute__((always_inline)) {
      const int n = c * 128 + wc * 32 + coff2;
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(q.b3 + n);
      const f32x4 b1 = *reinterpret_cast<const f32x4*>(q.b3 + n + 4);
      e_b3[0] = f32x2{b0[0], b0[1]}; e_b3[1] = f32x2{b0[2], b0[3]};
      e_b3[2] = f32x2{b1[0], b1[1]}; e_b3[3] = f32x2{b1[2], b1[3]};
    };
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) load_w(0, ks);
    load_res(0, P0{});
    load_res(1, P1{});
    __syncthreads();                                // the t2 slice is complete

    // the pixel fragments roll too: fragment i of K slice ks + 1 is read into xf[i] right after
    // the two MFMAs that consumed it for slice ks (and slice 0 again, for the next chunk, after
    // slice 7), so every ds_read has seven block pairs of MFMA work to return.  The scheduling
    // barriers pin that order; the compiler's own counted waits follow from it.
    // four address registers (K-slice parity x ring half); the rest are 16-bit immediates
    const bf16_t* xa[2][2];
#pragma unroll
    for (int par = 0; par < 2; ++par)
#pragma unroll
      for (int half = 0; half < 2; ++half)
        xa[par][half] = ring + half * 2 * T2_BLOCK + x_r0 + (((fq2 + 4 * par) ^ sw2) << 3);
    auto read_x = [&](int ks, int i) __attribute__((always_inline)) {
      return *reinterpret_cast<const bf16x8*>(xa[ks & 1][ks >> 2] + ((ks >> 1) & 1) * T2_BLOCK + i * 16 * 64);
    };
    bf16x8 xf[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) xf[i] = read_x(0, i);
    auto chunk = [&](int c, auto par_tag) __attribute__((always_inline)) {
      constexpr int P = decltype(par_tag)::value;
      // the fragment reads do not depend on c: keep them from being hoisted out of the loop
      asm volatile("" ::: "memory");
      f32x4 acc2[2][MI];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < MI; ++i) acc2[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
      load_b3(c);
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc2[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wreg[ks & 3][j], xf[i], acc2[j][i], 0, 0, 0);
          xf[i] = read_x((ks + 1) & 7, i);
          __builtin_amdgcn_sched_barrier(0);
        }
        // the slice four ahead (the next chunk's, from slice 4 on) into the freed registers
        if (ks < 4) load_w(c, ks + 4);
        else load_w(c + 1, ks - 4);
        __builtin_amdgcn_sched_barrier(0);
      }
      const uint32_t cb = (uint32_t)c * 256u;
      uint32_t rs = row_step;
      asm volatile("" : "+s"(rs));
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        f32x4 lo = acc2[0][i], hi = acc2[1][i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(lo[e]), __float_as_uint(hi[e]), false, false);
          lo[e] = __uint_as_float(s[0]);
          hi[e] = __uint_as_float(s[1]);
        }
        // bias and residual as packed fp32 adds, ReLU on the rounded bf16 pairs (a signed 16-bit
        // max with 0 clears exactly the negative ones): the same bits as max(v, 0) before rounding
        const f32x2 v[4] = {f32x2{lo[0], lo[1]} + e_b3[0], f32x2{lo[2], lo[3]} + e_b3[1],
                            f32x2{hi[0], hi[1]} + e_b3[2], f32x2{hi[2], hi[3]} + e_b3[3]};
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const f32x2 r = {__uint_as_float(e_res[P][i][e] << 16), __uint_as_float(e_res[P][i][e] & 0xffff0000u)};
          const f32x2 t = v[e] + r;
          o[e] = relu_bf16x2(pack2(t[0], t[1]));
        }
        __builtin_amdgcn_raw_buffer_store_b128(o, ry, row0 + rs * i, cb, 0);
        // one row at a time: its temporaries die here.  A 16-byte store reads its data registers
        // after it issues, and the next row reuses them at once; the compiler's hazard pass counts
        // the scheduling barrier below as the wait state it owes (seen: the next VALU write landed
        // in rows 252-255 of the store), so the wait states are spelled out.
        asm volatile("s_nop 1");
        __builtin_amdgcn_sched_barrier(0);
      }
      load_res(c + 2, par_tag);                     // two chunks ahead, into the buffer just freed
    };
    for (int c = 0; c < nch; c += 2) {              // N % 256 == 0: an even number of chunks
      chunk(c, P0{});
      chunk(c + 1, P1{});
    }
    __syncthreads();                                // t2 reads done before the next tile's DMA
  }
}

}  // namespace aiko

// t1 [B, H, W, 256] NHWC; w2 [256][9 * 256] (tap-major); w3img the fragment image of W3 [N][256];
// res / y [B, H, W, N], all contiguous bf16; b2 [256], b3 [N] fp32.  grid: workgroups (0: one per
// 256-pixel tile; fewer: each walks tiles g, g + grid, ...).
extern "C" int aiko_conv3x3_exp(const void* t1, const void* w2, const float* b2, const void* w3img,
                                const float* b3, const void* res, void* y, int B, int H, int W, int N,
                                int grid, hipStream_t stream) {
  using namespace aiko;
  const long M = (long)B * H * W;
  if (N <= 0 || N % 256 || M <= 0 || M * N * 2 >= 0x7ffffff0L || H * W <= 0 || grid < 0) return -1;
  ConvExpParams q;
  ConvParams& p = q.c;
  p.x = static_cast<const bf16_t*>(t1);
  p.w = static_cast<const bf16_t*>(w2);
  p.bias = b2;
  p.res = static_cast<const bf16_t*>(res);
  p.y = static_cast<bf16_t*>(y);
  p.H = H; p.W = W; p.C = 256; p.Cc = 256; p.R = 3; p.S = 3;
  p.stride = 1; p.pad = 1; p.Ho = H; p.Wo = W; p.M = (int)M; p.Cout = 256; p.K = 9 * 256;
  p.act = 1; p.ldy = N; p.ldr = N;
  p.x2 = nullptr;
  p.K1 = p.K; p.H2 = 0; p.W2 = 0; p.C2 = 0; p.stride2 = 1;
  conv_params_finalize(p);
  q.w3 = static_cast<const bf16_t*>(w3img);
  q.b3 = b3;
  q.N = N;
  const int ntiles = (int)((M + 255) / 256);
  const int g = grid > 0 && grid < ntiles ? grid : ntiles;
  conv3x3_exp_kernel<<<dim3(g), 512, 0, stream>>>(q);
  return (int)hipGetLastError();
}
