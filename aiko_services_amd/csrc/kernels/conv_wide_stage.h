// Staging primitives shared by the wide-tile implicit-GEMM kernels (conv_wide.hip, conv_exp.hip):
// raw buffer resources whose out-of-range offsets read as zero (the convolution's padding and
// the M tail), the 16-byte global -> LDS DMA, and the counted vmcnt wait + barrier.
#pragma once
#include "conv_common.h"

namespace aiko {

constexpr uint32_t kWideOOB = 0x80000000u;        // offsets >= num_records read as zero
constexpr uint32_t kWideRecords = 0x7ffffff0u;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t wide_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)kWideRecords, 0x00020000);
}

__device__ __forceinline__ void wide_dma16(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, void* lds) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(
      r, reinterpret_cast<__attribute__((address_space(3))) void*>(reinterpret_cast<uintptr_t>(lds)), 16,
      voff, soff, 0, 0);
}

template <int N>
__device__ __forceinline__ void wide_vm_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

}  // namespace aiko
