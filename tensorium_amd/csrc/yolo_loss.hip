// yolo_loss.hip — the training part of TYoloLayer.forward (nyololayer.pas:
// 835-1003 with processBatch 500-774, deltaBox 124-202, deltaClass 204-251,
// averageDeltas 253-269, compareClass 272-281, getBox 105-122 and box_iou,
// ntypes.pas:1059-1108, in yolo_box.hpp) for one [yolo] layer, on the device: truth boxes in,
// the layer's delta and cost[0] out.  Scope: iou_loss=mse, iou_thresh_kind=
// iou, scale_x_y=1, none of focal_loss / objectness_smooth / label_smooth_eps
// / new_coords / counters_per_class / map / embedding_layer, [net] without
// adversarial and without the bad-label rejection keys ("The YOLO
// loss").
//
// Four stages in stream order:
//   cell pass      one thread per (image, anchor, cell), lines 535-632; every
//                  write lands in the thread's own cell, delta.fill(0) folded
//                  in (each thread writes all classes+5 entries of its cell);
//   truth pass     one wave per image walks the truths in order, lines
//                  633-761; every delta element is read and written by one
//                  fixed lane (box entry k: lane k, objectness: lane 0, class
//                  c: lane c mod 64), so program order is the only order
//                  needed;
//   averaging pass lines 762-773, only when iou_thresh < 1, per cell;
//   cost           delta.sumSquares() = TTensor<T>.sumSqr (ntensors.pas:
//                  9333-9341): one ascending chain sum := sum + x*x.  A zero
//                  element adds +0 and the chain never holds -0, so the chain
//                  runs over the non-zero elements only: count per block,
//                  scan, ordered compaction of the squares, then one wave
//                  adding them one rounding at a time.
//
// Numerics (the file is compiled with -ffp-contract=off):
// FPC's exp / ln return a real (double here), so an expression that holds one
// is evaluated in double from there on and rounded once where it is assigned
// to a single; every other expression is single with each operation rounded.
// The type of each sub-expression stands next to it: [s] single, [d] double.
#include "tns_internal.hpp"
#include "yolo_box.hpp"

namespace tns {
namespace {

// getBox (nyololayer.pas:105-122), not newCoords, from the cell's four box
// entries o[0..3]
__device__ __forceinline__ Box get_box(const YoloLossParams& p, const float o[4], int an, int col,
                                       int row) {
  Box b;
  b.x = ((float)col + o[0]) / (float)p.w;  // [s] (col + out) [s] / w [s]
  b.y = ((float)row + o[1]) / (float)p.h;  // [s]
  // exp(out) [d] * bias [d] / netWidth [d], rounded on the assignment
  b.w = (float)(exp((double)o[2]) * (double)p.biases[2 * an] / (double)p.netW);
  b.h = (float)(exp((double)o[3]) * (double)p.biases[2 * an + 1] / (double)p.netH);
  return b;
}

// deltaBox's mse targets (nyololayer.pas:147-150) for anchor an at cell (i, j)
__device__ __forceinline__ void box_targets(const YoloLossParams& p, const Box& t, int an, int i,
                                            int j, float tg[4]) {
  tg[0] = t.x * (float)p.w - (float)i;  // [s] product [s], difference [s]
  tg[1] = t.y * (float)p.h - (float)j;  // [s]
  // ln(truth.w * w / bias): the argument [s] (product, quotient), ln [d],
  // rounded on the assignment to tw
  tg[2] = (float)log((double)(t.w * (float)p.w / p.biases[2 * an]));
  tg[3] = (float)log((double)(t.h * (float)p.h / p.biases[2 * an + 1]));
}

// class_id := trunc(truth[4]) in [0, classes): trunc rounds toward zero, so
// exactly the values in (-1, classes); NaN names no class
__device__ __forceinline__ bool class_valid(float cf, int classes) {
  return cf > -1.0f && cf < (float)classes;
}

__device__ __forceinline__ bool finite_f(float v) {
  return fabsf(v) <= 3.402823466e+38f;  // false for NaN and +-Inf
}

// ---- cell pass -------------------------------------------------------------
// grid (ceil(hw / 256), anchors, batch); dynamic LDS: the image's truth rows
__global__ void __launch_bounds__(256)
yolo_cell_kernel(YoloLossParams p, float* __restrict__ out, const float* __restrict__ truth,
                 float* __restrict__ delta, unsigned long long* __restrict__ counters) {
  extern __shared__ float s_truth[];  // [maxBoxes][6]
  __shared__ int s_nt, s_any;
  const int b = blockIdx.z, a = blockIdx.y;
  const int hw = p.h * p.w;
  const float* tr = truth + (int64_t)b * p.maxBoxes * 6;
  if (threadIdx.x == 0) {
    s_nt = p.maxBoxes;
    s_any = 0;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < p.maxBoxes * 6; k += blockDim.x) s_truth[k] = tr[k];
  // the first row with x == 0 ends the list
  for (int t = threadIdx.x; t < p.maxBoxes; t += blockDim.x)
    if (tr[6 * t] == 0.0f) atomicMin(&s_nt, t);
  __syncthreads();
  const int nt = s_nt;
  for (int t = threadIdx.x; t < nt; t += blockDim.x)
    if (class_valid(s_truth[6 * t + 4], p.classes)) atomicOr(&s_any, 1);
  __syncthreads();
  const bool any_valid = s_any != 0;  // the truth loop reaches a valid truth
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= hw) return;
  const int row = cell / p.w, col = cell - row * p.w;
  const int64_t stride = hw;
  const int64_t base = ((int64_t)(b * p.n + a) * (p.classes + 5)) * stride + cell;
  const int an = p.mask[a];
  float ob[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) ob[k] = out[base + k * stride];
  const Box pred = get_box(p, ob, an, col, row);
  float obj = out[base + 4 * stride];
  bool match = false;  // compareClass(class_index, stride, 0.25)
  if (any_valid) {
    // the reference resets a NaN / Inf objectness inside the truth loop, at
    // the first truth with a valid class (lines 559-561)
    if (!finite_f(obj)) {
      obj = 0.0f;
      out[base + 4 * stride] = 0.0f;
    }
    for (int c = 0; c < p.classes; ++c)
      if (out[base + (5 + c) * stride] > 0.25f) match = true;
  }
  float best_match_iou = 0.0f, best_iou = 0.0f;
  int best_t = 0;
  for (int t = 0; t < nt; ++t) {
    const float* r = s_truth + 6 * t;
    if (!class_valid(r[4], p.classes)) continue;
    const Box tb{r[0], r[1], r[2], r[3]};
    const float iou = box_iou(pred, tb);
    if (iou > best_match_iou && match) best_match_iou = iou;
    if (iou > best_iou) {
      best_iou = iou;
      best_t = t;
    }
  }
  float dobj = p.objNormalizer * (-obj);  // [s]
  if (best_match_iou > p.ignoreThresh) dobj = 0.0f;
  float dbox[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int cls = -1;
  if (best_iou > p.truthThresh) {
    // (best_t stays 0 when no truth overlapped: the reference then takes row
    // 0 whatever its class; a class outside [0, classes) would index outside
    // the cell, so such a row is not taken)
    const float* r = s_truth + 6 * best_t;
    if (class_valid(r[4], p.classes)) {
      cls = (int)r[4];
      dobj = p.objNormalizer * (1.0f - obj);  // [s] (1 - out) [s], product [s]
      const Box tb{r[0], r[1], r[2], r[3]};
      const float scale = 2.0f - tb.w * tb.h;  // [s]
      float tg[4];
      box_targets(p, tb, an, col, row, tg);
#pragma unroll
      for (int k = 0; k < 4; ++k)  // delta (0 here) + scale*(t - out)*iou_normalizer, all [s]
        dbox[k] = 0.0f + scale * (tg[k] - ob[k]) * p.iouNormalizer;
      atomicAdd(&counters[0], 1ull);  // inc(net.totalBBox)
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) delta[base + k * stride] = dbox[k];
  delta[base + 4 * stride] = dobj;
  for (int c = 0; c < p.classes; ++c) {
    float d = 0.0f;
    if (cls >= 0) {  // deltaClass, second branch: y_true - out unless NaN / Inf
      const float rd = (c == cls ? 1.0f : 0.0f) - out[base + (5 + c) * stride];  // [s]
      if (finite_f(rd)) d = rd;
    }
    delta[base + (5 + c) * stride] = d;
  }
}

// ---- truth pass ------------------------------------------------------------
// one truth's writes on cell (i, j) of mask entry mask_n for anchor an:
// deltaBox (mse, accumulate), the objectness delta, deltaClass.  Returns the
// IoU of the predicted box (all_ious.iou); *rewritten: the four box deltas
// were not all zero before.  All lanes of the wave call it together.
__device__ __forceinline__ float truth_write(const YoloLossParams& p,
                                             const float* __restrict__ out, float* delta, int b,
                                             int mask_n, int an, int i, int j, const Box& t,
                                             int cls, bool* rewritten) {
  const int lane = threadIdx.x;
  const int64_t stride = (int64_t)p.h * p.w;
  const int64_t base = ((int64_t)(b * p.n + mask_n) * (p.classes + 5)) * stride + j * p.w + i;
  const int owner = cls & 63;
  const int64_t cidx = base + 5 * stride;
  // every load of this write is issued here, before the first use: one
  // memory latency a truth, not one a step
  float dk = 0.0f, dcur = 0.0f, oc0 = 0.0f;
  if (lane < 4) dk = delta[base + lane * stride];
  if (lane == owner) dcur = delta[cidx + cls * stride];
  float ob[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) ob[k] = out[base + k * stride];
  const float oobj = out[base + 4 * stride];
  const float ocls = out[cidx + cls * stride];
  if (lane < p.classes) oc0 = out[cidx + lane * stride];
  const float scale = 2.0f - t.w * t.h;  // [s]
  *rewritten = __ballot(lane < 4 && dk != 0.0f) != 0ull;
  const Box pred = get_box(p, ob, an, i, j);
  const float iou = box_iou(pred, t);
  float tg[4];
  box_targets(p, t, an, i, j, tg);
  if (lane < 4) {
    const float tk = lane == 0 ? tg[0] : lane == 1 ? tg[1] : lane == 2 ? tg[2] : tg[3];
    const float ok = lane == 0 ? ob[0] : lane == 1 ? ob[1] : lane == 2 ? ob[2] : ob[3];
    // delta + scale * (t - out) * iou_normalizer, every operation [s]
    delta[base + lane * stride] = dk + scale * (tk - ok) * p.iouNormalizer;
  }
  // class_multiplier (1) * obj_normalizer * (1 - out), [s]
  if (lane == 0) delta[base + 4 * stride] = p.objNormalizer * (1.0f - oobj);
  // deltaClass: a class delta that is already non-zero is the only one rewritten
  const bool first = __ballot(lane == owner && dcur != 0.0f) != 0ull;
  if (first) {
    if (lane == owner) {
      const float rd = 1.0f - ocls;  // [s]
      if (finite_f(rd)) delta[cidx + cls * stride] = rd;
    }
  } else {
    for (int c = lane; c < p.classes; c += 64) {
      const float oc = c == lane ? oc0 : out[cidx + c * stride];
      const float rd = (c == cls ? 1.0f : 0.0f) - oc;  // [s]
      if (finite_f(rd)) delta[cidx + c * stride] = rd;
    }
  }
  return iou;
}

__device__ __forceinline__ int mask_index_of(const YoloLossParams& p, int an) {
  for (int k = 0; k < p.n; ++k)
    if (p.mask[k] == an) return k;
  return -1;
}

// grid (batch), one wave each
__global__ void __launch_bounds__(64)
yolo_truth_kernel(YoloLossParams p, const float* __restrict__ out,
                  const float* __restrict__ truth, float* delta, float* __restrict__ stats,
                  unsigned long long* __restrict__ counters) {
  extern __shared__ float s_rows[];  // the image's truth rows, [maxBoxes][6]
  const int b = blockIdx.x, lane = threadIdx.x;
  for (int k = lane; k < p.maxBoxes * 6; k += 64)
    s_rows[k] = truth[(int64_t)b * p.maxBoxes * 6 + k];
  __syncthreads();
  const float* tr = s_rows;
  float tot_iou = 0.0f;  // args.tot_iou: one running single sum, in truth order
  int count = 0;
  unsigned long long total_bbox = 0, rewritten_bbox = 0;
  for (int t = 0; t < p.maxBoxes; ++t) {
    const Box tb{tr[6 * t], tr[6 * t + 1], tr[6 * t + 2], tr[6 * t + 3]};
    if (tb.x == 0.0f) break;
    const float cf = tr[6 * t + 4];
    if (!class_valid(cf, p.classes)) continue;
    const int cls = (int)cf;
    // i := trunc(truth.x * w), j := trunc(truth.y * h) [s products].  The
    // reference indexes that cell unchecked; a truth whose cell lies outside
    // the grid is skipped here (DESIGN.md quirk list)
    const float fi = tb.x * (float)p.w, fj = tb.y * (float)p.h;
    if (!(fi > -1.0f && fi < (float)p.w && fj > -1.0f && fj < (float)p.h)) continue;
    const int i = (int)fi, j = (int)fj;
    const Box shift{0.0f, 0.0f, tb.w, tb.h};
    float best_iou = 0.0f;
    int best_n = 0;
    for (int n = 0; n < p.total; ++n) {
      // pred.w := biases[2n] / netWidth, [s]
      const Box pa{0.0f, 0.0f, p.biases[2 * n] / (float)p.netW,
                   p.biases[2 * n + 1] / (float)p.netH};
      const float iou = box_iou(pa, shift);
      if (iou > best_iou) {
        best_iou = iou;
        best_n = n;
      }
    }
    const int mask_n = mask_index_of(p, best_n);
    if (mask_n >= 0) {
      bool rew;
      const float iou = truth_write(p, out, delta, b, mask_n, best_n, i, j, tb, cls, &rew);
      rewritten_bbox += rew ? 1 : 0;
      ++total_bbox;
      tot_iou = tot_iou + iou;  // [s]
      ++count;
    }
    if (p.iouThresh < 1.0f) {
      for (int n = 0; n < p.total; ++n) {
        const int mn = mask_index_of(p, n);
        if (mn < 0 || n == best_n) continue;
        const Box pa{0.0f, 0.0f, p.biases[2 * n] / (float)p.netW,
                     p.biases[2 * n + 1] / (float)p.netH};
        if (box_iou(pa, shift) > p.iouThresh) {
          bool rew;
          const float iou = truth_write(p, out, delta, b, mn, n, i, j, tb, cls, &rew);
          rewritten_bbox += rew ? 1 : 0;
          ++total_bbox;
          tot_iou = tot_iou + iou;  // [s]
          ++count;
        }
      }
    }
  }
  if (lane == 0) {
    if (stats) {
      stats[2 * b] = (float)count;
      stats[2 * b + 1] = tot_iou;
    }
    if (total_bbox) atomicAdd(&counters[0], total_bbox);
    if (rewritten_bbox) atomicAdd(&counters[1], rewritten_bbox);
  }
}

// ---- averaging pass (iou_thresh < 1) -----------------------------------------
// averageDeltas on every cell whose objectness delta is non-zero
__global__ void __launch_bounds__(256)
yolo_average_kernel(YoloLossParams p, float* __restrict__ delta) {
  const int b = blockIdx.z, a = blockIdx.y;
  const int hw = p.h * p.w;
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= hw) return;
  const int64_t stride = hw;
  const int64_t base = ((int64_t)(b * p.n + a) * (p.classes + 5)) * stride + cell;
  if (!(delta[base + 4 * stride] != 0.0f)) return;
  int in_box = 0;  // classes_in_one_box
  for (int c = 0; c < p.classes; ++c)
    if (delta[base + (5 + c) * stride] > 0.0f) ++in_box;
  if (in_box > 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      delta[base + k * stride] = delta[base + k * stride] / (float)in_box;  // [s]
  }
}

// ---- cost --------------------------------------------------------------------
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

// cost[0] = ((0 + sq[0]) + sq[1]) + ..., one rounding per add.  One wave: its
// lanes bring tiles of 1024 squares into LDS with coalesced loads, two tiles
// ahead of the chain; every lane then reads the tile by broadcast and runs
// the same chain, one dependent add an element.
__global__ void __launch_bounds__(64)
cost_chain_kernel(const float* __restrict__ sq, const int* __restrict__ m_ptr,
                  float* __restrict__ cost) {
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
  if (lane == 0) cost[0] = sum;
}

}  // namespace

int64_t yolo_loss_scratch_floats(int64_t n) {
  const int64_t nb = (n + kChunk - 1) / kChunk;
  return n + 2 * nb + 2;  // the squares, counts[nb], offsets[nb + 1]
}

hipError_t launch_yolo_loss(const YoloLossParams& p, float* out, const float* truth, float* delta,
                            float* cost, float* stats, unsigned long long* counters,
                            float* scratch, hipStream_t s) {
  const int hw = p.h * p.w;
  const int64_t n = (int64_t)p.batch * p.n * (p.classes + 5) * hw;
  const dim3 cells((hw + 255) / 256, p.n, p.batch);
  hipLaunchKernelGGL(yolo_cell_kernel, cells, dim3(256), (size_t)p.maxBoxes * 6 * sizeof(float), s,
                     p, out, truth, delta, counters);
  hipLaunchKernelGGL(yolo_truth_kernel, dim3(p.batch), dim3(64),
                     (size_t)p.maxBoxes * 6 * sizeof(float), s, p, out, truth, delta, stats,
                     counters);
  if (p.iouThresh < 1.0f)
    hipLaunchKernelGGL(yolo_average_kernel, cells, dim3(256), 0, s, p, delta);
  const int nb = (int)((n + kChunk - 1) / kChunk);
  float* sq = scratch;
  int* counts = reinterpret_cast<int*>(scratch + n);
  int* offsets = counts + nb;
  hipLaunchKernelGGL(cost_count_kernel, dim3(nb), dim3(256), 0, s, n, delta, counts);
  hipLaunchKernelGGL(cost_scan_kernel, dim3(1), dim3(1024), 0, s, nb, counts, offsets);
  hipLaunchKernelGGL(cost_compact_kernel, dim3(nb), dim3(256), 0, s, n, delta, offsets, sq);
  hipLaunchKernelGGL(cost_chain_kernel, dim3(1), dim3(64), 0, s, sq, offsets + nb, cost);
  return hipGetLastError();
}

}  // namespace tns
