// detections.hip — what the reference's detection sample does after the
// forward pass, on the device:
//
//   collect  TYoloLayer.getDetectionCount / getDetections / correctBoxes
//            (nyololayer.pas:378-498, getBox 105-122) for one [yolo] layer and
//            all images: the candidates (cell i, anchor a) whose objectness is
//            > thresh become rows {bbox, objectness, prob[classes]}, in the
//            reference's order (cell outer, anchor inner), appended behind the
//            rows an earlier layer left (the per-image device counter);
//   nms      TDetections.doNMSSort (ntypes.pas:1554-1565, 1612-1649) on such a
//            buffer, in place on prob.
//
// Collect is an ordered compaction in three launches: the taken candidates of
// every 256-candidate chunk are counted, one block an image scans the chunk
// counts behind the image's counter (and adds the total to it), and every
// chunk then writes its rows from its own offset.  A row's place is the
// number of taken candidates before it, whatever the schedule.
//
// NMS runs one workgroup per (image, class).  The rows that take part
// (objectness != 0) and whose prob[k] is not +0 are gathered as 64-bit keys
// (score descending, row ascending) and sorted in LDS; their boxes follow in
// sorted order, and the walk costs one barrier per surviving row while all
// lanes test the later rows.  kNmsLds keys fit; a class with more takes the
// second form, which needs no storage: it finds the next live key above the
// last one by a block-wide minimum and zeroes the later rows it overlaps,
// straight on global memory.  Both forms visit the live rows in the same
// order, so they give the same bits.
//
// Numerics (compiled with -ffp-contract=off): exp returns
// a real (double) and its expression stays double until it is assigned to a
// single; integer / integer is a real; everything else is single with every
// operation rounded.  [s] single, [d] double, [i] integer.
#include "tns_internal.hpp"
#include "yolo_box.hpp"

namespace tns {
namespace {

constexpr int kDetChunk = 256;  // candidates per block of the collect kernels
constexpr int kNmsThreads = 256;
constexpr int kNmsLds = 2048;  // candidates of one (image, class) the sorted form holds

// ---- collect ---------------------------------------------------------------
// candidate c of an image = (cell c / n, anchor c % n): cell outer, anchor
// inner, the reference's loop order (nyololayer.pas:412-416)
__device__ __forceinline__ int64_t det_entry(const DetParams& p, int b, int a, int cell, int entry) {
  return ((int64_t)(b * p.n + a) * (p.classes + 5) + entry) * ((int64_t)p.h * p.w) + cell;
}

// objectness > thresh, strict; false for NaN (lines 392-394, 424-426)
__device__ __forceinline__ bool det_taken(const DetParams& p, const float* __restrict__ out,
                                          int b, int c) {
  if (c >= p.h * p.w * p.n) return false;
  return out[det_entry(p, b, c % p.n, c / p.n, 4)] > p.thresh;
}

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

// grid (chunks, batch)
__global__ void __launch_bounds__(kDetChunk)
det_count_kernel(DetParams p, const float* __restrict__ out, int* __restrict__ chunk_counts) {
  const int b = blockIdx.y;
  int total;
  det_chunk_rank(det_taken(p, out, b, blockIdx.x * kDetChunk + threadIdx.x), &total);
  if (threadIdx.x == 0) chunk_counts[(int64_t)b * gridDim.x + blockIdx.x] = total;
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

// getBox (nyololayer.pas:105-122), not newCoords, then correctBoxes (452-498)
// on that one box
__device__ __forceinline__ Box det_box(const DetParams& p, const float o[4], int an, int col,
                                       int row) {
  Box b;
  b.x = ((float)col + o[0]) / (float)p.w;  // [s] (col + out) [s] / w [s]
  b.y = ((float)row + o[1]) / (float)p.h;  // [s]
  // exp(out) [d] * bias [d] / netWidth [d], rounded on the assignment
  b.w = (float)(exp((double)o[2]) * (double)p.biases[2 * an] / (double)p.netW);
  b.h = (float)(exp((double)o[3]) * (double)p.biases[2 * an + 1] / (double)p.netH);
  // correctBoxes: w, h are the image's extents from here on
  long long new_w = p.netW, new_h = p.netH;  // [i]
  if (p.letter) {
    // (netw / w) [d] < (neth / h) [d]: integer / integer is a real
    if ((double)p.netW / (double)p.imW < (double)p.netH / (double)p.imH)
      new_h = ((long long)p.imH * p.netW) / p.imW;  // [i] (h * netw) div w
    else
      new_w = ((long long)p.imW * p.netH) / p.imH;  // [i] (w * neth) div h
  }
  const float deltaw = (float)(p.netW - new_w);  // [i] difference, assigned to a single
  const float deltah = (float)(p.netH - new_h);
  const float ratiow = (float)((double)new_w / (double)p.netW);  // [d] quotient, rounded once
  const float ratioh = (float)((double)new_h / (double)p.netH);
  // (b.x - deltaw / 2.0 / netw) / ratiow: deltaw / 2.0 [s], / netw [s], the
  // difference [s], / ratiow [s]
  b.x = (b.x - deltaw / 2.0f / (float)p.netW) / ratiow;
  b.y = (b.y - deltah / 2.0f / (float)p.netH) / ratioh;
  b.w = b.w * (1.0f / ratiow);  // (1 / ratiow) [s], the product [s]
  b.h = b.h * (1.0f / ratioh);
  if (!p.relative) {
    b.x = b.x * (float)p.imW;  // [s] single * integer
    b.w = b.w * (float)p.imW;
    b.y = b.y * (float)p.imH;
    b.h = b.h * (float)p.imH;
  }
  return b;
}

// grid (chunks, batch)
__global__ void __launch_bounds__(kDetChunk)
det_fill_kernel(DetParams p, const float* __restrict__ out,
                const long long* __restrict__ chunk_offsets, float* __restrict__ boxes,
                float* __restrict__ objectness, float* __restrict__ probs) {
  __shared__ int s_cand[kDetChunk];
  const int b = blockIdx.y;
  const int c = blockIdx.x * kDetChunk + threadIdx.x;
  const bool taken = det_taken(p, out, b, c);
  int total;
  const int rank = det_chunk_rank(taken, &total);
  if (taken) s_cand[rank] = c;
  __syncthreads();
  // the chunk's first row; rows outside [0, capacity) are counted, not written
  const long long first = chunk_offsets[(int64_t)b * gridDim.x + blockIdx.x];
  if ((int)threadIdx.x < total) {
    const long long r = first + threadIdx.x;
    if (r >= 0 && r < p.capacity) {
      const int cand = s_cand[threadIdx.x];
      const int a = cand % p.n, cell = cand / p.n;
      float o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = out[det_entry(p, b, a, cell, k)];
      const Box bx = det_box(p, o, p.mask[a], cell % p.w, cell / p.w);
      float* dst = boxes + ((int64_t)b * p.capacity + r) * 4;
      dst[0] = bx.x, dst[1] = bx.y, dst[2] = bx.w, dst[3] = bx.h;
      objectness[(int64_t)b * p.capacity + r] = out[det_entry(p, b, a, cell, 4)];
    }
  }
  // prob[j] = objectness * class_j if > thresh, else 0 (lines 435-443); class
  // fastest, so a row's probabilities are written side by side
  for (int64_t e = threadIdx.x; e < (int64_t)total * p.classes; e += kDetChunk) {
    const int local = (int)(e / p.classes), j = (int)(e - (int64_t)local * p.classes);
    const long long r = first + local;
    if (r < 0 || r >= p.capacity) continue;
    const int cand = s_cand[local];
    const int a = cand % p.n, cell = cand / p.n;
    const float prob = out[det_entry(p, b, a, cell, 4)] * out[det_entry(p, b, a, cell, 5 + j)];  // [s]
    probs[((int64_t)b * p.capacity + r) * p.classes + j] = prob > p.thresh ? prob : 0.0f;
  }
}

// ---- NMS -------------------------------------------------------------------
// Comparer's order (ntypes.pas:1554-1565) made total: ascending keys are
// descending scores, equal scores by ascending row.  -0 orders just below +0
// and above every negative score.
__device__ __forceinline__ unsigned long long nms_key(float score, int row) {
  const unsigned int u = __float_as_uint(score);
  const unsigned int ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending with the score
  return ((unsigned long long)(~ord) << 32) | (unsigned int)row;
}

__device__ __forceinline__ Box nms_box(const float* __restrict__ boxes, int64_t row) {
  const float* s = boxes + row * 4;
  return Box{s[0], s[1], s[2], s[3]};
}

// the block's smallest v (every thread gets it)
__device__ __forceinline__ unsigned long long nms_block_min(unsigned long long v) {
  __shared__ unsigned long long s_min[kNmsThreads / 64];
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d, 64);
    v = o < v ? o : v;
  }
  __syncthreads();  // (the last call's reads of s_min are over)
  if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = v;
  __syncthreads();
  v = s_min[0];
#pragma unroll
  for (int k = 1; k < kNmsThreads / 64; ++k) v = s_min[k] < v ? s_min[k] : v;
  return v;
}

// the second form: no list.  Each round takes the live row (prob[k] != 0)
// with the smallest key above the last one taken and zeroes the rows after it
// that it overlaps.  A thread reads and writes only the rows r = threadIdx.x
// mod kNmsThreads, so program order is the only order prob needs.
__device__ void nms_unsorted(int n, int classes, int k, const float* __restrict__ boxes,
                             const float* __restrict__ obj, float* probs, float thresh) {
  unsigned long long cur = 0;
  bool first = true;
  for (;;) {
    unsigned long long best = ~0ull;
    for (int r = threadIdx.x; r < n; r += kNmsThreads) {
      if (obj[r] == 0.0f) continue;
      const float s = probs[(int64_t)r * classes + k];
      if (!(s != 0.0f)) continue;
      const unsigned long long key = nms_key(s, r);
      if ((first || key > cur) && key < best) best = key;
    }
    best = nms_block_min(best);
    if (best == ~0ull) return;
    const Box a = nms_box(boxes, (int64_t)(best & 0xffffffffull));
    for (int r = threadIdx.x; r < n; r += kNmsThreads) {
      if (obj[r] == 0.0f) continue;
      const float s = probs[(int64_t)r * classes + k];
      if (__float_as_uint(s) == 0u) continue;  // +0 stays +0
      if (nms_key(s, r) > best && box_iou(a, nms_box(boxes, r)) > thresh)
        probs[(int64_t)r * classes + k] = 0.0f;
    }
    cur = best;
    first = false;
  }
}

// grid (classes, batch)
__global__ void __launch_bounds__(kNmsThreads)
nms_sort_kernel(int capacity, int classes, const long long* __restrict__ counts,
                const float* __restrict__ boxes_all, const float* __restrict__ obj_all,
                float* probs_all, float thresh) {
  __shared__ unsigned long long s_key[kNmsLds];
  __shared__ Box s_box[kNmsLds];
  __shared__ unsigned char s_live[kNmsLds], s_supp[kNmsLds];
  __shared__ int s_m;
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const long long cnt = counts[b];
  const int n = cnt < 0 ? 0 : cnt < capacity ? (int)cnt : capacity;
  const float* boxes = boxes_all + (int64_t)b * capacity * 4;
  const float* obj = obj_all + (int64_t)b * capacity;
  float* probs = probs_all + (int64_t)b * capacity * classes;
  if (tid == 0) s_m = 0;
  __syncthreads();
  // the rows that take part (objectness != 0, lines 1619-1633) and whose
  // prob[k] is not +0: a +0 row suppresses nothing and zeroing it changes
  // nothing.  (The order of the gather does not matter: the keys are distinct
  // and sorted next.)
  for (int r = tid; r < n; r += kNmsThreads) {
    if (obj[r] == 0.0f) continue;
    const float s = probs[(int64_t)r * classes + k];
    if (__float_as_uint(s) == 0u) continue;
    const int at = atomicAdd(&s_m, 1);
    if (at < kNmsLds) s_key[at] = nms_key(s, r);
  }
  __syncthreads();
  const int m = s_m;
  if (m == 0) return;
  if (m > kNmsLds) {
    nms_unsorted(n, classes, k, boxes, obj, probs, thresh);
    return;
  }
  int pow2 = 1;
  while (pow2 < m) pow2 <<= 1;
  for (int i = m + tid; i < pow2; i += kNmsThreads) s_key[i] = ~0ull;
  __syncthreads();
  for (int size = 2; size <= pow2; size <<= 1)  // bitonic sort, ascending
    for (int d = size >> 1; d > 0; d >>= 1) {
      for (int i = tid; i < pow2; i += kNmsThreads) {
        const int j = i ^ d;
        if (j > i) {
          const unsigned long long x = s_key[i], y = s_key[j];
          if ((x > y) == ((i & size) == 0)) {
            s_key[i] = y;
            s_key[j] = x;
          }
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < m; i += kNmsThreads) {
    const int64_t r = (int64_t)(s_key[i] & 0xffffffffull);
    s_box[i] = nms_box(boxes, r);
    s_live[i] = probs[r * classes + k] != 0.0f ? 1 : 0;  // (-0 is not live)
    s_supp[i] = 0;
  }
  __syncthreads();
  // lines 1639-1647: a row still non-zero zeroes every later row it overlaps;
  // one barrier per such row
  for (int i = 0; i < m; ++i) {
    if (!s_live[i] || s_supp[i]) continue;
    const Box a = s_box[i];
    for (int j = i + 1 + tid; j < m; j += kNmsThreads)
      if (!s_supp[j] && box_iou(a, s_box[j]) > thresh) s_supp[j] = 1;
    __syncthreads();
  }
  for (int i = tid; i < m; i += kNmsThreads)
    if (s_supp[i]) probs[(int64_t)(s_key[i] & 0xffffffffull) * classes + k] = 0.0f;
}

}  // namespace

int64_t detections_scratch_floats(const DetParams& p) {
  const int64_t chunks = ((int64_t)p.h * p.w * p.n + kDetChunk - 1) / kDetChunk;
  return 3 * chunks * p.batch;  // offsets (int64), then counts (int)
}

hipError_t launch_yolo_detections(const DetParams& p, const float* out, int64_t* counts,
                                  float* boxes, float* objectness, float* probs, float* scratch,
                                  hipStream_t s) {
  const int chunks = (int)(((int64_t)p.h * p.w * p.n + kDetChunk - 1) / kDetChunk);
  if (chunks == 0 || p.batch == 0) return hipSuccess;
  long long* offsets = reinterpret_cast<long long*>(scratch);
  int* chunk_counts = reinterpret_cast<int*>(offsets + (int64_t)chunks * p.batch);
  const dim3 grid(chunks, p.batch);
  hipLaunchKernelGGL(det_count_kernel, grid, dim3(kDetChunk), 0, s, p, out, chunk_counts);
  hipLaunchKernelGGL(det_scan_kernel, dim3(p.batch), dim3(256), 0, s, chunks, chunk_counts,
                     offsets, reinterpret_cast<long long*>(counts));
  hipLaunchKernelGGL(det_fill_kernel, grid, dim3(kDetChunk), 0, s, p, out, offsets, boxes,
                     objectness, probs);
  return hipGetLastError();
}

hipError_t launch_nms_sort(int batch, int capacity, int classes, const int64_t* counts,
                           const float* boxes, const float* objectness, float* probs,
                           float thresh, hipStream_t s) {
  if (batch == 0 || classes == 0) return hipSuccess;
  hipLaunchKernelGGL(nms_sort_kernel, dim3(classes, batch), dim3(kNmsThreads), 0, s, capacity,
                     classes, reinterpret_cast<const long long*>(counts), boxes, objectness,
                     probs, thresh);
  return hipGetLastError();
}

}  // namespace tns
