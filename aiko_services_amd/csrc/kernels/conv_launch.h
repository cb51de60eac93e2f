// Host-side launch description shared by the implicit-GEMM conv launchers and the binding
// (plain C++, no device types).
#pragma once
#include <hip/hip_runtime_api.h>

// tile=(bm, bn, variant): mirrors ``Variant`` / ``VARIANTS`` in ops/conv.py, which holds each
// kernel's tile list and the measurements behind its default / opt-in status.  The numbers are a
// persisted format (tile caches, profiles): never re-used.  10, 16 and 17 (conv_patch / patchw /
// rows) have operators of their own and are listed for completeness.
enum ConvVariant {
  CONV_IGEMM = 0,           // conv_igemm.hip: register-staged
  CONV_GLDS = 1,            // conv_glds.hip: LDS-DMA, padding read from a zero page
  CONV_BUF = 2,             // conv_buf.hip: buffer LDS-DMA, padding by out-of-range reads
  CONV_BUF_OCC = 3,         //   at forced high occupancy (64x64: 5, 64x128 / 128x64: 3 per CU)
  CONV_PERSIST = 4,         // conv_persist.hip: one K-block stream across a workgroup's tiles
  CONV_BUF_MF32 = 5,        // conv_buf.hip on the 32x32x16 MFMA
  CONV_BUF_WIDE4 = 6,       //   as 4-wave 256x128 / 128x256 tiles
  CONV_NARROW = 7,          // conv_narrow.hip: direct kernel, Cc and Cout in {16, 32}
  CONV_WIDE = 8,            // conv_wide.hip: 8 waves, register-direct epilogue
  CONV_WIDE_OCC = 9,        //   at 2-3 workgroups per CU
  CONV_PATCH = 10,
  CONV_WIDE_DEEP = 11,      //   32-deep K blocks in a 4-slot ring
  CONV_PW = 12,             // conv_pw.hip: persistent pointwise GEMM
  CONV_PW_RESIDENT = 13,    //   weight block resident in LDS (with x2: the fused projection)
  CONV_PW_RESIDENT_AB = 14, //   residual issued at its own tile
  CONV_PATCHW = 16,
  CONV_ROWS = 17,
  CONV_WIDE_EXACT_N = 18,   // conv_wide.hip: bn = 80 / 144 channels computed per tile
  CONV_WIDE4_OCC = 19,      //   4 waves of 64x64 / 64x128
  CONV_WIDE_PERSIST = 20,   //   persistent walk over the tiles
};

struct ConvLaunch {
  const void* x;
  const void* w;       // [Cout][K] bf16
  const float* bias;   // [Cout] or nullptr
  const void* res;     // [M][ldr] or nullptr
  void* y;             // [M][ldy]
  int H, W, C, Cc, R, S, stride, pad, Ho, Wo, M, Cout, K, act, ldy, ldr;
  int bm, bn;          // block tile
  const void* x2;      // optional second A source (K columns [K1, K)), see ConvParams
  int K1, H2, W2, C2, stride2;
  hipStream_t stream;
};
