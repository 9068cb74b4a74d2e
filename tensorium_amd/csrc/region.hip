// region.hip — TRegionLayer (nregionlayer.pas), YOLOv2's head, on the device.
// The reference runs the layer on the CPU only (no forwardGPU).  Built:
// coords = 4, no softmax tree, no map, no focal loss ("The region
// layer").  size = classes + 5, C = n * size channels.
//
//   forward     lines 297-325 with flatten (97-116) and softmax (129-152) in
//               one kernel.  A block owns T consecutive cells of one image:
//               their output is one contiguous span of T*C floats.  Each
//               channel row's T floats come in coalesced and go to LDS as
//               tile[c][t], row stride T + 1: odd, so the walk of one thread
//               per (cell, anchor) down its column meets no bank twice among
//               the lanes of consecutive cells.  The logistic of entry 4 and
//               the class softmax run there, classes in the reference's order;
//               the span goes out with 16-byte stores between its first and
//               last 16-byte boundary.  T is the largest power of two up to 32
//               whose tile fits kRegionLds (32 for VOC's 125 and COCO's 425
//               channels); the last tile of an image is short.
//   loss        lines 328-480, into a flattened delta held in scratch:
//     cell pass   one thread per (image, cell, anchor), lines 367-418; every
//                 write lands in the thread's own cell, delta.fill(0) folded
//                 in (each thread writes all size entries);
//     truth pass  one wave per image walks the truths in order, lines
//                 419-475; the anchor search runs with lanes over anchors;
//                 box entry k is written by lane k, the objectness by lane 0,
//                 class c by lane c mod 64, and the pass reads no delta, so
//                 program order is the only order needed;
//     un-flatten  the forward tile run backwards: span in, channel rows out,
//                 into the caller's delta [batch][C][hw];
//     cost        sqr(delta.sumSquares()) over that order: ordered_cost.hpp.
//   detections  getDetections + getBoxes + correct_yolo_boxes, lines 534-690:
//               count, scan (det_scan.hpp), fill, as detections.hip.
//
// Numerics (compiled with -ffp-contract=off): exp / ln
// return a real (double), so an expression that holds one is double from
// there on and rounded once where it is assigned to a single (a function
// result of type single is such an assignment); everything else is single
// with each operation rounded.  [s] single, [d] double.
#include "tns_internal.hpp"

// every device function of this file, the shared stages included, is compiled
// without packed single-precision operations: each operation stands alone
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "det_scan.hpp"
#include "ordered_cost.hpp"
#include "yolo_box.hpp"

namespace tns {
namespace {

constexpr int kTileThreads = 256;

// logistic_activate (118-122), result single: -x [s], exp [d], 1 + e [d],
// 1 / that [d], rounded on return
__device__ __forceinline__ float logistic(float x) {
  return (float)(1.0 / (1.0 + exp((double)(-x))));
}

// logistic_gradient (124-127): (1 - x) [s] * x [s]
__device__ __forceinline__ float logistic_gradient(float x) { return (1.0f - x) * x; }

// ---- the tile ----------------------------------------------------------------
// tile[c * S + t], S = T + 1; tv <= T cells of it are inside the image.
// rows: element (c, t) at rows[c * hw + t]; span: at span[t * C + c].
__device__ __forceinline__ void rows_to_lds(const float* __restrict__ rows, int hw, int C,
                                            int tshift, int tv, float* tile) {
  const int T = 1 << tshift, S = T + 1;
  for (int e = threadIdx.x; e < C << tshift; e += kTileThreads) {
    const int c = e >> tshift, t = e & (T - 1);
    if (t < tv) tile[c * S + t] = rows[(int64_t)c * hw + t];
  }
}

__device__ __forceinline__ void lds_to_rows(float* __restrict__ rows, int hw, int C, int tshift,
                                            int tv, const float* tile) {
  const int T = 1 << tshift, S = T + 1;
  for (int e = threadIdx.x; e < C << tshift; e += kTileThreads) {
    const int c = e >> tshift, t = e & (T - 1);
    if (t < tv) rows[(int64_t)c * hw + t] = tile[c * S + t];
  }
}

__device__ __forceinline__ int span_slot(int o, int C, int S) {
  const int t = o / C;
  return (o - t * C) * S + t;
}

// the floats before the first 16-byte boundary of a 4-byte aligned pointer
__device__ __forceinline__ int span_head(const float* sp, int len) {
  const int head = (4 - (int)(((uintptr_t)sp >> 2) & 3)) & 3;
  return head < len ? head : len;
}

__device__ __forceinline__ void lds_to_span(float* __restrict__ sp, int len, int C, int S,
                                            const float* tile) {
  const int head = span_head(sp, len), body = (len - head) >> 2, done = head + 4 * body;
  if ((int)threadIdx.x < head) sp[threadIdx.x] = tile[span_slot(threadIdx.x, C, S)];
  for (int q = threadIdx.x; q < body; q += kTileThreads) {
    const int o = head + 4 * q;
    *reinterpret_cast<float4*>(sp + o) =
        make_float4(tile[span_slot(o, C, S)], tile[span_slot(o + 1, C, S)],
                    tile[span_slot(o + 2, C, S)], tile[span_slot(o + 3, C, S)]);
  }
  if ((int)threadIdx.x < len - done)
    sp[done + threadIdx.x] = tile[span_slot(done + threadIdx.x, C, S)];
}

__device__ __forceinline__ void span_to_lds(const float* __restrict__ sp, int len, int C, int S,
                                            float* tile) {
  const int head = span_head(sp, len), body = (len - head) >> 2, done = head + 4 * body;
  if ((int)threadIdx.x < head) tile[span_slot(threadIdx.x, C, S)] = sp[threadIdx.x];
  for (int q = threadIdx.x; q < body; q += kTileThreads) {
    const int o = head + 4 * q;
    const float4 v = *reinterpret_cast<const float4*>(sp + o);
    tile[span_slot(o, C, S)] = v.x;
    tile[span_slot(o + 1, C, S)] = v.y;
    tile[span_slot(o + 2, C, S)] = v.z;
    tile[span_slot(o + 3, C, S)] = v.w;
  }
  if ((int)threadIdx.x < len - done)
    tile[span_slot(done + threadIdx.x, C, S)] = sp[done + threadIdx.x];
}

// ---- forward -----------------------------------------------------------------
// grid (ceil(hw / T), batch); dynamic LDS: C * (T + 1) floats
__global__ void __launch_bounds__(kTileThreads)
region_forward_kernel(int n, int classes, int hw, int tshift, int softmax,
                      const float* __restrict__ in, float* __restrict__ out) {
  extern __shared__ float tile[];
  const int size = classes + 5, C = n * size, T = 1 << tshift, S = T + 1;
  const int b = blockIdx.y, cell0 = blockIdx.x << tshift;
  const int tv = hw - cell0 < T ? hw - cell0 : T;
  rows_to_lds(in + (int64_t)b * C * hw + cell0, hw, C, tshift, tv, tile);
  __syncthreads();
  for (int u = threadIdx.x; u < n << tshift; u += kTileThreads) {
    const int a = u >> tshift, t = u & (T - 1);
    if (t >= tv) continue;
    float* col = tile + a * size * S + t;  // entry k of (cell t, anchor a) at col[k * S]
    col[4 * S] = logistic(col[4 * S]);
    if (softmax && classes > 0) {  // softmax(input, classes, temp = 1, output, 1)
      float* x = col + 5 * S;
      float largest = x[0];
      for (int i = 1; i < classes; ++i)
        if (x[i * S] > largest) largest = x[i * S];
      float sum = 0.0f;
      for (int i = 0; i < classes; ++i) {
        // (x - largest) [s] / temp [s] (temp = 1), exp [d], rounded into e
        const float e = (float)exp((double)((x[i * S] - largest) / 1.0f));
        sum = sum + e;  // [s]
        x[i * S] = e;
      }
      for (int i = 0; i < classes; ++i) x[i * S] = x[i * S] / sum;  // [s]
    }
  }
  __syncthreads();
  lds_to_span(out + ((int64_t)b * hw + cell0) * C, tv * C, C, S, tile);
}

// ---- loss --------------------------------------------------------------------
// getBox (498-509) from the raw entries o[0..3] of anchor an at (col, row);
// netWidth / netHeight are the layer's w / h at every call
__device__ __forceinline__ Box region_box(const RegionParams& p, const float o[4], int an, int col,
                                          int row) {
  Box b;
  b.x = ((float)col + logistic(o[0])) / (float)p.w;  // [s] (col + single) [s] / w [s]
  b.y = ((float)row + logistic(o[1])) / (float)p.h;  // [s]
  // exp(out) [d] * bias [d] / netWidth [d], rounded on the assignment
  b.w = (float)(exp((double)o[2]) * (double)p.biases[2 * an] / (double)p.w);
  b.h = (float)(exp((double)o[3]) * (double)p.biases[2 * an + 1] / (double)p.h);
  return b;
}

// deltaBox (511-532): the four box deltas d[] of anchor an at (col, row) for
// `truth`; returns pred.iou(truth)
__device__ __forceinline__ float delta_box(const RegionParams& p, const Box& truth,
                                           const float o[4], int an, int col, int row, float scale,
                                           float d[4]) {
  const float iou = box_iou(region_box(p, o, an, col, row), truth);
  const float tx = truth.x * (float)p.w - (float)col;  // [s] product, difference
  const float ty = truth.y * (float)p.h - (float)row;  // [s]
  // ln(truth.w * w / bias): the argument [s] (product, quotient), ln [d],
  // rounded on the assignment to tw
  const float tw = (float)log((double)(truth.w * (float)p.w / p.biases[2 * an]));
  const float th = (float)log((double)(truth.h * (float)p.h / p.biases[2 * an + 1]));
  const float lx = logistic(o[0]), ly = logistic(o[1]);
  d[0] = scale * (tx - lx) * logistic_gradient(lx);  // [s], left to right
  d[1] = scale * (ty - ly) * logistic_gradient(ly);
  d[2] = scale * (tw - o[2]);  // [s]
  d[3] = scale * (th - o[3]);
  return iou;
}

// a truth row's class passes `class_id >= classes -> continue` (class_id :=
// trunc(row[4])): exactly the values below classes; NaN names no class
__device__ __forceinline__ bool class_kept(float cf, int classes) { return cf < (float)classes; }

// trunc(cf) as the index delta_region_class compares with: a negative
// class_id matches no class
__device__ __forceinline__ int class_index(float cf) { return cf <= -1.0f ? -1 : (int)cf; }

// grid (ceil(hw * n / 256), batch); dynamic LDS: the image's truth rows
__global__ void __launch_bounds__(256)
region_cell_kernel(RegionParams p, const float* __restrict__ out, const float* __restrict__ truth,
                   float* __restrict__ flat) {
  extern __shared__ float s_truth[];  // [maxBoxes][6]
  const int b = blockIdx.y, hw = p.h * p.w, size = p.classes + 5;
  for (int k = threadIdx.x; k < p.maxBoxes * 6; k += blockDim.x)
    s_truth[k] = truth[(int64_t)b * p.maxBoxes * 6 + k];
  __syncthreads();
  const int u = blockIdx.x * blockDim.x + threadIdx.x;  // cell * n + anchor
  if (u >= hw * p.n) return;
  const int cell = u / p.n, a = u - cell * p.n;
  const int row = cell / p.w, col = cell - row * p.w;
  const int64_t index = ((int64_t)b * hw * p.n + u) * size;
  float o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = out[index + k];
  const float obj = out[index + 4];
  const Box pred = region_box(p, o, a, col, row);
  float best_iou = 0.0f;
  int best_cls = -1;
  for (int t = 0; t < p.maxBoxes; ++t) {
    const float* r = s_truth + 6 * t;
    if (!class_kept(r[4], p.classes)) continue;  // before the x = 0 test, as the reference
    if (r[0] == 0.0f) break;
    const float iou = box_iou(pred, Box{r[0], r[1], r[2], r[3]});
    if (iou > best_iou) {
      best_cls = class_index(r[4]);
      best_iou = iou;
    }
  }
  const float grad = logistic_gradient(obj);
  float dobj = p.noobjectScale * ((-obj) * grad);  // [s]
  bool classes_on = false;
  float cscale = 0.0f;
  if (p.classfix == -1) {
    dobj = p.noobjectScale * ((best_iou - obj) * grad);  // [s]
  } else if (best_iou > p.thresh) {
    dobj = 0.0f;
    if (p.classfix > 0) {
      classes_on = true;
      cscale = p.classScale * (p.classfix == 2 ? obj : 1.0f);  // [s]
    }
  }
  float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (p.prior) {  // state.seen^ < 12800: the prior box at scale 0.01
    Box tr;
    tr.x = ((float)col + 0.5f) / (float)p.w;  // (i + 0.5) exact, one rounded quotient
    tr.y = ((float)row + 0.5f) / (float)p.h;
    tr.w = p.biases[2 * a] / (float)p.w;  // [s]
    tr.h = p.biases[2 * a + 1] / (float)p.h;
    delta_box(p, tr, o, a, col, row, 0.01f, d);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) flat[index + k] = d[k];
  flat[index + 4] = dobj;
  for (int c = 0; c < p.classes; ++c)  // delta_region_class, flat branch: scale * (y - out) [s]
    flat[index + 5 + c] =
        classes_on ? cscale * ((c == best_cls ? 1.0f : 0.0f) - out[index + 5 + c]) : 0.0f;
}

// grid (batch), one wave each; dynamic LDS: the image's truth rows
__global__ void __launch_bounds__(64)
region_truth_kernel(RegionParams p, const float* __restrict__ out, const float* __restrict__ truth,
                    float* flat) {
  extern __shared__ float s_rows[];  // [maxBoxes][6]
  const int b = blockIdx.x, lane = threadIdx.x;
  const int hw = p.h * p.w, size = p.classes + 5;
  for (int k = lane; k < p.maxBoxes * 6; k += 64)
    s_rows[k] = truth[(int64_t)b * p.maxBoxes * 6 + k];
  __syncthreads();
  for (int t = 0; t < p.maxBoxes; ++t) {
    const float* r = s_rows + 6 * t;
    if (!class_kept(r[4], p.classes)) continue;
    if (r[0] == 0.0f) break;
    const int cls = class_index(r[4]);
    const Box tb{r[0], r[1], r[2], r[3]};
    // i := trunc(truth.x * w), j := trunc(truth.y * h) [s products]; a cell
    // outside the grid is skipped (the reference indexes it unchecked)
    const float fi = tb.x * (float)p.w, fj = tb.y * (float)p.h;
    if (!(fi > -1.0f && fi < (float)p.w && fj > -1.0f && fj < (float)p.h)) continue;
    const int i = (int)fi, j = (int)fj;
    const int64_t cbase = ((int64_t)b * hw + j * p.w + i) * p.n * size;  // the cell's anchor 0
    // the anchor whose box, moved to the origin, overlaps the truth's most:
    // lane a holds anchor a's iou; the first of the largest wins, as the
    // ascending loop's `iou > best_iou` has it, anchor 0 when none is above 0
    float mine = 0.0f;
    if (lane < p.n) {
      Box pr{0.0f, 0.0f, 0.0f, 0.0f};
      if (p.biasMatch) {
        pr.w = p.biases[2 * lane] / (float)p.w;  // [s]
        pr.h = p.biases[2 * lane + 1] / (float)p.h;
      } else {  // getBox's w, h: exp(out) [d] * bias [d] / w [d], rounded once
        const float* oa = out + cbase + lane * size;
        pr.w = (float)(exp((double)oa[2]) * (double)p.biases[2 * lane] / (double)p.w);
        pr.h = (float)(exp((double)oa[3]) * (double)p.biases[2 * lane + 1] / (double)p.h);
      }
      const float iou = box_iou(pr, Box{0.0f, 0.0f, tb.w, tb.h});
      mine = iou > 0.0f ? iou : 0.0f;
    }
    float top = mine;
    for (int d = 32; d > 0; d >>= 1) {
      const float other = __shfl_xor(top, d, 64);
      top = other > top ? other : top;
    }
    const unsigned long long hit = __ballot(lane < p.n && mine == top);
    const int best_n = top > 0.0f ? __ffsll((long long)hit) - 1 : 0;
    const int64_t index = cbase + best_n * size;
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = out[index + k];
    const float obj = out[index + 4];
    float d[4];
    const float iou = delta_box(p, tb, o, best_n, i, j, p.coordScale, d);
    const float grad = logistic_gradient(obj);
    float dobj = p.objectScale * (1.0f - obj) * grad;          // [s], left to right
    if (p.rescore) dobj = p.objectScale * (iou - obj) * grad;  // [s]
    if (lane < 4) flat[index + lane] = lane == 0 ? d[0] : lane == 1 ? d[1] : lane == 2 ? d[2] : d[3];
    if (lane == 0) flat[index + 4] = dobj;
    for (int c = lane; c < p.classes; c += 64)  // delta_region_class, flat branch
      flat[index + 5 + c] = p.classScale * ((c == cls ? 1.0f : 0.0f) - out[index + 5 + c]);
  }
}

// grid (ceil(hw / T), batch); dynamic LDS: C * (T + 1) floats.  flatten(delta,
// forward = false): flat [batch][hw][C] to delta [batch][C][hw]
__global__ void __launch_bounds__(kTileThreads)
region_unflatten_kernel(int C, int hw, int tshift, const float* __restrict__ flat,
                        float* __restrict__ delta) {
  extern __shared__ float tile[];
  const int T = 1 << tshift, S = T + 1;
  const int b = blockIdx.y, cell0 = blockIdx.x << tshift;
  const int tv = hw - cell0 < T ? hw - cell0 : T;
  span_to_lds(flat + ((int64_t)b * hw + cell0) * C, tv * C, C, S, tile);
  __syncthreads();
  lds_to_rows(delta + (int64_t)b * C * hw + cell0, hw, C, tshift, tv, tile);
}

// ---- detections ----------------------------------------------------------------
// candidate u of an image = (cell u / n, anchor u % n), the flattened order
// and getBoxes' loop order (546-552)
__device__ __forceinline__ float det_scale(const RegionParams& p, float obj) {
  return (p.classfix == -1 && obj < 0.5f) ? 0.0f : obj;  // lines 554-556
}

// at least one prob[j] = scale * class_j [s] is > thresh (strict; false for NaN)
__device__ __forceinline__ bool region_taken(const RegionParams& p, const float* __restrict__ out,
                                             int b, int u) {
  const int cands = p.h * p.w * p.n;
  if (u >= cands) return false;
  const float* o = out + ((int64_t)b * cands + u) * (p.classes + 5);
  const float scale = det_scale(p, o[4]);
  for (int j = 0; j < p.classes; ++j)
    if (scale * o[5 + j] > p.thresh) return true;
  return false;
}

// grid (chunks, batch)
__global__ void __launch_bounds__(kDetChunk)
region_det_count_kernel(RegionParams p, const float* __restrict__ out,
                        int* __restrict__ chunk_counts) {
  const int b = blockIdx.y;
  int total;
  det_chunk_rank(region_taken(p, out, b, blockIdx.x * kDetChunk + threadIdx.x), &total);
  if (threadIdx.x == 0) chunk_counts[(int64_t)b * gridDim.x + blockIdx.x] = total;
}

// grid (chunks, batch)
__global__ void __launch_bounds__(kDetChunk)
region_det_fill_kernel(RegionParams p, const float* __restrict__ out,
                       const long long* __restrict__ chunk_offsets, float* __restrict__ boxes,
                       float* __restrict__ objectness, float* __restrict__ probs) {
  __shared__ int s_cand[kDetChunk];
  const int b = blockIdx.y, size = p.classes + 5;
  const int u = blockIdx.x * kDetChunk + threadIdx.x;
  const bool taken = region_taken(p, out, b, u);
  int total;
  const int rank = det_chunk_rank(taken, &total);
  if (taken) s_cand[rank] = u;
  __syncthreads();
  const float* img = out + (int64_t)b * p.h * p.w * p.n * size;
  // the chunk's first row; rows outside [0, capacity) are counted, not written
  const long long first = chunk_offsets[(int64_t)b * gridDim.x + blockIdx.x];
  if ((int)threadIdx.x < total) {
    const long long r = first + threadIdx.x;
    if (r >= 0 && r < p.capacity) {
      const int cand = s_cand[threadIdx.x];
      const int cell = cand / p.n, a = cand - cell * p.n;
      // getBox, times aWidth = aHeight = 1 (exact), then correct_yolo_boxes
      const Box bx = correct_box(region_box(p, img + (int64_t)cand * size, a, cell % p.w, cell / p.w),
                                 p.netW, p.netH, p.imW, p.imH, p.relative, p.letter);
      float* dst = boxes + ((int64_t)b * p.capacity + r) * 4;
      dst[0] = bx.x, dst[1] = bx.y, dst[2] = bx.w, dst[3] = bx.h;
      objectness[(int64_t)b * p.capacity + r] = 1.0f;  // dets[j].objectness := 1
    }
  }
  // prob[j] = scale * class_j if > thresh, else 0 (593-600); a row's
  // probabilities are read and written side by side
  for (int64_t e = threadIdx.x; e < (int64_t)total * p.classes; e += kDetChunk) {
    const int local = (int)(e / p.classes), j = (int)(e - (int64_t)local * p.classes);
    const long long r = first + local;
    if (r < 0 || r >= p.capacity) continue;
    const float* o = img + (int64_t)s_cand[local] * size;
    const float prob = det_scale(p, o[4]) * o[5 + j];  // [s]
    probs[((int64_t)b * p.capacity + r) * p.classes + j] = prob > p.thresh ? prob : 0.0f;
  }
}

int tile_shift(int64_t channels) {
  for (int s = 5; s >= 0; --s)
    if (channels * ((1 << s) + 1) * (int64_t)sizeof(float) <= kRegionLds) return s;
  return -1;
}

size_t tile_bytes(int64_t channels, int shift) {
  return (size_t)channels * ((1 << shift) + 1) * sizeof(float);
}

int64_t det_chunks(const RegionParams& p) {
  return ((int64_t)p.h * p.w * p.n + kDetChunk - 1) / kDetChunk;
}

// the cost stage's scratch, rounded up to whole 16 bytes; flat follows it
int64_t cost_floats(int64_t n) { return (ordered_cost_scratch_floats(n) + 3) & ~(int64_t)3; }

}  // namespace

int region_tile_cells(int64_t channels) {
  const int s = tile_shift(channels);
  return s < 0 ? 0 : 1 << s;
}

hipError_t launch_region_forward(int batch, int n, int classes, int hw, int softmax,
                                 const float* in, float* out, hipStream_t s) {
  const int C = n * (classes + 5), shift = tile_shift(C);
  const dim3 grid((hw + (1 << shift) - 1) >> shift, batch);
  hipLaunchKernelGGL(region_forward_kernel, grid, dim3(kTileThreads), tile_bytes(C, shift), s, n,
                     classes, hw, shift, softmax, in, out);
  return hipGetLastError();
}

int64_t region_loss_scratch_floats(int64_t n) { return cost_floats(n) + n; }

hipError_t launch_region_loss(const RegionParams& p, const float* out, const float* truth,
                              float* delta, float* cost, float* scratch, hipStream_t s) {
  const int hw = p.h * p.w, C = p.n * (p.classes + 5), shift = tile_shift(C);
  const int64_t n = (int64_t)p.batch * C * hw;
  float* flat = scratch + cost_floats(n);
  const size_t rows = (size_t)p.maxBoxes * 6 * sizeof(float);
  hipLaunchKernelGGL(region_cell_kernel, dim3((hw * p.n + 255) / 256, p.batch), dim3(256), rows, s,
                     p, out, truth, flat);
  hipLaunchKernelGGL(region_truth_kernel, dim3(p.batch), dim3(64), rows, s, p, out, truth, flat);
  hipLaunchKernelGGL(region_unflatten_kernel, dim3((hw + (1 << shift) - 1) >> shift, p.batch),
                     dim3(kTileThreads), tile_bytes(C, shift), s, C, hw, shift, flat, delta);
  launch_ordered_cost(n, delta, cost, scratch, true, s);
  return hipGetLastError();
}

int64_t region_detections_scratch_floats(const RegionParams& p) {
  return det_scan_scratch_floats(det_chunks(p), p.batch);
}

hipError_t launch_region_detections(const RegionParams& p, const float* out, int64_t* counts,
                                    float* boxes, float* objectness, float* probs,
                                    float* scratch, hipStream_t s) {
  const int chunks = (int)det_chunks(p);
  if (chunks == 0 || p.batch == 0) return hipSuccess;
  long long* offsets = reinterpret_cast<long long*>(scratch);
  int* chunk_counts = reinterpret_cast<int*>(offsets + (int64_t)chunks * p.batch);
  const dim3 grid(chunks, p.batch);
  hipLaunchKernelGGL(region_det_count_kernel, grid, dim3(kDetChunk), 0, s, p, out, chunk_counts);
  hipLaunchKernelGGL(det_scan_kernel, dim3(p.batch), dim3(256), 0, s, chunks, chunk_counts, offsets,
                     reinterpret_cast<long long*>(counts));
  hipLaunchKernelGGL(region_det_fill_kernel, grid, dim3(kDetChunk), 0, s, p, out, offsets, boxes,
                     objectness, probs);
  return hipGetLastError();
}

}  // namespace tns

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
