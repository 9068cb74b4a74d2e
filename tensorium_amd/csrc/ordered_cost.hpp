// ordered_cost.hpp — delta.sumSquares() = TTensor<T>.sumSqr (ntensors.pas:
// 9333-9341) in the reference's order, the cost stage shared by yolo_loss.hip
// and region.hip: one ascending chain sum := sum + x*x.  A zero element adds
// +0 and the chain never holds -0, so the chain runs over the non-zero
// elements only: count per block, scan, ordered compaction of the squares,
// then one wave adding them one rounding at a time.  Compiled with
// -ffp-contract=off; [s] marks a single.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tns {
namespace {

constexpr int kPerThread = 8;
constexpr int kChunk = 256 * kPerThread;  // elements per block, thread-contiguous

// the exclusive offset of this thread's non-zeros within its block's chunk and
// (in *block_total) the chunk's count; v: the thread's elements, 0 past n
__device__ __forceinline__ int chunk_offsets(int64_t n, const float* __restrict__ x,
                                             float v[kPerThread], int* block_total) {
  __shared__ int s_cnt[256];
  const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * kPerThread;
  int mine = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    v[k] = first + k < n ? x[first + k] : 0.0f;
    mine += v[k] != 0.0f ? 1 : 0;  // (NaN counts: it takes part in the chain)
  }
  s_cnt[threadIdx.x] = mine;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {  // inclusive scan
    const int add = (int)threadIdx.x >= d ? s_cnt[threadIdx.x - d] : 0;
    __syncthreads();
    s_cnt[threadIdx.x] += add;
    __syncthreads();
  }
  *block_total = s_cnt[255];
  return s_cnt[threadIdx.x] - mine;
}

__global__ void __launch_bounds__(256)
cost_count_kernel(int64_t n, const float* __restrict__ x, int* __restrict__ counts) {
  float v[kPerThread];
  int total;
  chunk_offsets(n, x, v, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one block: offsets[i] = counts[0] + .. + counts[i-1], offsets[nb] = the total
__global__ void __launch_bounds__(1024)
cost_scan_kernel(int nb, const int* __restrict__ counts, int* __restrict__ offsets) {
  __shared__ int s[1024];
  __shared__ int s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int i0 = 0; i0 < nb; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const int mine = i < nb ? counts[i] : 0;
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const int add = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    const int carry = s_carry;
    if (i < nb) offsets[i] = carry + s[threadIdx.x] - mine;
    __syncthreads();
    if (threadIdx.x == 1023) s_carry = carry + s[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) offsets[nb] = s_carry;
}

// sq[position among the non-zeros] = x*x [s], in index order
__global__ void __launch_bounds__(256)
cost_compact_kernel(int64_t n, const float* __restrict__ x, const int* __restrict__ offsets,
                    float* __restrict__ sq) {
  float v[kPerThread];
  int total;
  int at = offsets[blockIdx.x] + chunk_offsets(n, x, v, &total);
#pragma unroll
  for (int k = 0; k < kPerThread; ++k)
    if (v[k] != 0.0f) sq[at++] = v[k] * v[k];
}

// four squares from element e on (e a multiple of 4, sq 16-byte aligned); +0
// past the end, which leaves the sum as it is
__device__ __forceinline__ float4 load_squares(const float* __restrict__ sq, int e, int m) {
  if (e + 3 < m) return *reinterpret_cast<const float4*>(sq + e);
  return make_float4(e < m ? sq[e] : 0.0f, e + 1 < m ? sq[e + 1] : 0.0f,
                     e + 2 < m ? sq[e + 2] : 0.0f, 0.0f);
}

// cost[0] = ((0 + sq[0]) + sq[1]) + ..., one rounding per add; with `squared`
// that sum times itself [s] (TRegionLayer's sqr(delta.sumSquares())).  One
// wave: its lanes bring tiles of 1024 squares into LDS with coalesced loads,
// two tiles ahead of the chain; every lane then reads the tile by broadcast
// and runs the same chain, one dependent add an element.
__global__ void __launch_bounds__(64)
cost_chain_kernel(const float* __restrict__ sq, const int* __restrict__ m_ptr,
                  float* __restrict__ cost, int squared) {
  __shared__ float4 tile[2][256];
  const int m = *m_ptr, lane = threadIdx.x;
  const int ntiles = (m + 1023) / 1024;
  float4 a[4], b[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    a[q] = load_squares(sq, (q * 64 + lane) * 4, m);
    b[q] = load_squares(sq, 1024 + (q * 64 + lane) * 4, m);
  }
  float sum = 0.0f;
  for (int t = 0; t < ntiles; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      tile[t & 1][q * 64 + lane] = a[q];
      a[q] = b[q];
      b[q] = load_squares(sq, (t + 2) * 1024 + (q * 64 + lane) * 4, m);
    }
    __syncthreads();  // (one wave: the tile written above is visible below; the
                      // other tile is rewritten only after the next barrier)
    const float4* tp = tile[t & 1];
#pragma unroll 8
    for (int q = 0; q < 256; ++q) {
      const float4 v = tp[q];
      sum = sum + v.x;  // [s]
      sum = sum + v.y;
      sum = sum + v.z;
      sum = sum + v.w;
    }
  }
  if (lane == 0) cost[0] = squared ? sum * sum : sum;
}

// scratch floats for n elements: the squares, counts[nb], offsets[nb + 1]
inline int64_t ordered_cost_scratch_floats(int64_t n) {
  const int64_t nb = (n + kChunk - 1) / kChunk;
  return n + 2 * nb + 2;
}

// the four launches, n > 0
inline void launch_ordered_cost(int64_t n, const float* x, float* cost, float* scratch,
                                bool squared, hipStream_t s) {
  const int nb = (int)((n + kChunk - 1) / kChunk);
  float* sq = scratch;
  int* counts = reinterpret_cast<int*>(scratch + n);
  int* offsets = counts + nb;
  hipLaunchKernelGGL(cost_count_kernel, dim3(nb), dim3(256), 0, s, n, x, counts);
  hipLaunchKernelGGL(cost_scan_kernel, dim3(1), dim3(1024), 0, s, nb, counts, offsets);
  hipLaunchKernelGGL(cost_compact_kernel, dim3(nb), dim3(256), 0, s, n, x, offsets, sq);
  hipLaunchKernelGGL(cost_chain_kernel, dim3(1), dim3(64), 0, s, sq, offsets + nb, cost,
                     squared ? 1 : 0);
}

}  // namespace
}  // namespace tns
