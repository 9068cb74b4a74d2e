// conv_bf16_common.hpp — what the bf16 MFMA convolution kernels share
// (conv_bf16.hip, conv_bf16_bwd.hip, conv_bf16_train.hip): the vector types,
// the LDS row geometry, the float -> bf16 rounding and the 16-byte LDS store of
// rounded pairs.
// Device code only; include it inside the file's no-packed-fp32-ops region.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tns {
namespace bf16k {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kStep = 32;       // k per LDS stage
constexpr int kRow = 80;        // LDS bytes per row: 64 of data, 16 of padding
constexpr int kPackRows = 128;  // packed A rows are padded to the tallest tile
constexpr int kThreads = 256;

// float to bf16, nearest even, Inf kept, NaN kept (quiet): the integer form,
// whatever the denormal mode
__device__ __forceinline__ unsigned bf16_rne(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// two floats rounded into one bf16 pair, lo in the low half (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned bf16_pair(float lo, float hi) {
  const f32x2 p = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(p, bf16x2));
}

// KPT consecutive k of one row, rounded (v_cvt_pk_bf16_f32), as 16-byte pieces
template <int KPT>
__device__ __forceinline__ void store_b(unsigned char* row, const float (&g)[KPT]) {
#pragma unroll
  for (int q = 0; q < KPT / 8; ++q) {
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = bf16_pair(g[8 * q + 2 * j], g[8 * q + 2 * j + 1]);
    reinterpret_cast<uint4*>(row)[q] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace bf16k
}  // namespace tns
