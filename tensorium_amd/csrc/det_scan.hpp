// det_scan.hpp — the ordered scan behind the detection rows, shared by
// detections.hip ([yolo]) and region.hip ([region]): the taken candidates of
// every kDetChunk-candidate chunk are ranked, one block an image scans the
// chunk counts behind the image's counter (and adds the total to it).  A
// row's place is the number of taken candidates before it, whatever the
// schedule.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tns {
namespace {

constexpr int kDetChunk = 256;  // candidates per block of the collect kernels

// the taken candidates of this block's chunk before this thread's, and the
// chunk's total
__device__ __forceinline__ int det_chunk_rank(bool taken, int* total) {
  __shared__ int s_wave[kDetChunk / 64];
  const unsigned long long m = __ballot(taken);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kDetChunk / 64; ++k) {
    if (k < wave) before += s_wave[k];
    all += s_wave[k];
  }
  *total = all;
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

// grid (batch): chunk_offsets[b][c] = counts[b] + the chunks before c; then
// counts[b] += the image's taken candidates, fitting or not
__global__ void __launch_bounds__(256)
det_scan_kernel(int chunks, const int* __restrict__ chunk_counts,
                long long* __restrict__ chunk_offsets, long long* __restrict__ counts) {
  __shared__ int s[256];
  __shared__ long long s_carry;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) s_carry = counts[b];
  __syncthreads();
  for (int c0 = 0; c0 < chunks; c0 += 256) {
    const int c = c0 + threadIdx.x;
    const int mine = c < chunks ? chunk_counts[(int64_t)b * chunks + c] : 0;
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // inclusive scan
      const int add = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0;
      __syncthreads();
      s[threadIdx.x] += add;
      __syncthreads();
    }
    const long long carry = s_carry;
    if (c < chunks) chunk_offsets[(int64_t)b * chunks + c] = carry + s[threadIdx.x] - mine;
    __syncthreads();
    if (threadIdx.x == 255) s_carry = carry + s[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[b] = s_carry;
}

// scratch floats for `chunks` chunks of `batch` images: offsets (int64), then
// counts (int)
inline int64_t det_scan_scratch_floats(int64_t chunks, int64_t batch) {
  return 3 * chunks * batch;
}

}  // namespace
}  // namespace tns
