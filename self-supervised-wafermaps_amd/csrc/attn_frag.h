// Operand fragments of the bf16 attention kernels (attention.hip, interpret.hip): a head's [token][HD] rows as an
// LDS image padded to AT_ROWB bytes per row, and the mfma_f32_16x16x32_bf16 fragments read from it or from global
// memory.
#pragma once
#include "common.h"

namespace {

// LDS bytes per token row: HD bf16 + 16 B pad (144 for head dim 64, 80 for 32: in both, 16
// consecutive rows start on 16 distinct 4-bank groups)
#define AT_ROWB (HD * 2 + 16)

template <int HD>
__device__ __forceinline__ bf16x8_t frag_rows(const uint8_t* base, int row, int ks, int fg) {
  return *reinterpret_cast<const bf16x8_t*>(base + row * AT_ROWB + ks * 64 + fg * 16);
}

// One fragment (row, 32-wide k-slab ks, 16-byte piece fg) of a [token][HD] operand straight from global memory:
// what frag_rows reads from an LDS image.  Rows >= S read as zeros.  The forward kernel takes a strip's own query rows
// this way (only that wave uses them): the request is in flight under the K / V staging, and Q needs no LDS.
__device__ __forceinline__ bf16x8_t frag_global(const uint16_t* base, size_t row_stride, int row, int S, int ks, int fg) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (row < S) v = *reinterpret_cast<const uint4*>(base + (size_t)row * row_stride + ks * 32 + fg * 8);
  return __builtin_bit_cast(bf16x8_t, v);
}

// rows [0, S) of one [token][64] operand of (image b, head h) -> LDS; rows [S, SP) zero
template <int HD>
__device__ __forceinline__ void stage_rows(const uint16_t* src, size_t row_stride, int S, int SP, uint8_t* dst) {
  constexpr int CPR = HD / 8;  // 16-byte chunks per row
  for (int i = threadIdx.x; i < SP * CPR; i += blockDim.x) {
    const int r = i / CPR, c = i % CPR;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < S) v = *reinterpret_cast<const uint4*>(src + (size_t)r * row_stride + c * 8);
    *reinterpret_cast<uint4*>(dst + r * AT_ROWB + c * 16) = v;
  }
}

}  // namespace
