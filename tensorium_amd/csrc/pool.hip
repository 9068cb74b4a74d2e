// pool.hip — max and local-average pooling (TMaxPoolLayer, nMaxPoolLayer.pas):
// forwardMaxPool (415-451), forwardAvgPool (465-499) and the two backward
// loops (501-542), each as one fold over the same window walk.
//
// Forward: per output (p, i, j) the window is scanned rows outer, columns
// inner, from (off + i*stride_y, off + j*stride_x), off = -(padding div 2).
//   max: strict `val > max` from max = -FLT_MAX, max_i = -1.  An out-of-range
//        tap reads as -FLT_MAX and so never wins (max >= -FLT_MAX always):
//        it is skipped.  NaN and -inf never compare greater either.
//   avg: in-range taps summed in scan order (one rounding per add), then one
//        correctly rounded division by their count.
// Backward: a gather in the CPU's add order instead of the reference device
// kernel's scatter (several outputs may name one input when stride < size).
// One thread owns an input element, walks the outputs whose windows cover it
// with i ascending outer, j ascending inner — ascending output index, the
// order of the CPU loop — and adds, one rounding per add:
//   max: delta[out] where indexes[out] is this element's absolute index
//        (-1 names no element and is never matched);
//   avg: delta[out] / float(size*size) for every covering output.
// Nothing is written unless something was added.
//
// Indexing inside a plane is int, plane offsets and stored indexes int64.
// A thread handles 4 adjacent elements of one row, so that a wave's row
// accesses are contiguous; float4 / 2 x longlong2 where the row length and
// the pointers allow, scalar otherwise.
#include "tns_internal.hpp"

#include <cfloat>

namespace tns {
namespace {

constexpr int V = 4;  // adjacent elements of a row per thread

struct Fold {
  float acc[V];
  int best[V];  // max: in-plane index of the maximum; avg: in-range taps
};

template <bool AVG>
__device__ __forceinline__ void fold_init(Fold& f) {
#pragma unroll
  for (int v = 0; v < V; ++v) {
    f.acc[v] = AVG ? 0.0f : -FLT_MAX;
    f.best[v] = AVG ? 0 : -1;
  }
}
template <bool AVG>
__device__ __forceinline__ void fold_tap(Fold& f, int v, float val, int at) {
  if constexpr (AVG) {
    f.acc[v] = f.acc[v] + val;
    ++f.best[v];
  } else if (val > f.acc[v]) {
    f.acc[v] = val;
    f.best[v] = at;
  }
}
// the results of one thread: outputs [o, o + n) of the batch buffer; plane
// = first element of the input plane (the stored indexes are absolute)
template <bool AVG>
__device__ __forceinline__ void fold_store(const Fold& f, int n, int64_t o, int64_t plane,
                                           float* __restrict__ out, int64_t* __restrict__ idx,
                                           bool vec) {
  float r[V];
  long long ix[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    r[v] = AVG ? f.acc[v] / (float)f.best[v] : f.acc[v];
    ix[v] = f.best[v] < 0 ? -1ll : (long long)(plane + f.best[v]);
  }
  if (vec) {  // n == V, o % 4 == 0, aligned buffers
    *reinterpret_cast<float4*>(out + o) = make_float4(r[0], r[1], r[2], r[3]);
    if (!AVG && idx) {
      *reinterpret_cast<longlong2*>(idx + o) = make_longlong2(ix[0], ix[1]);
      *reinterpret_cast<longlong2*>(idx + o + 2) = make_longlong2(ix[2], ix[3]);
    }
    return;
  }
#pragma unroll
  for (int v = 0; v < V; ++v)
    if (v < n) {
      out[o + v] = r[v];
      if (!AVG && idx) idx[o + v] = ix[v];
    }
}

// any size / strides / padding: every tap bounds-checked
template <bool AVG>
__global__ __launch_bounds__(256) void pool_fwd_kernel(int64_t planes, PoolGeom g,
                                                       const float* __restrict__ in,
                                                       float* __restrict__ out,
                                                       int64_t* __restrict__ idx, int vec) {
  const int qw = (g.outW + V - 1) / V;
  const int64_t total = planes * g.outH * qw;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total;
       it += (int64_t)gridDim.x * blockDim.x) {
    const int j0 = (int)(it % qw) * V;
    const int64_t r = it / qw;  // output row (plane, i)
    const int i = (int)(r % g.outH);
    const int64_t plane = (r / g.outH) * g.h * g.w;
    const int n = g.outW - j0 < V ? g.outW - j0 : V;
    Fold f;
    fold_init<AVG>(f);
    const int h0 = g.off + i * g.sy;
    for (int kn = 0; kn < g.size; ++kn) {
      const int ch = h0 + kn;
      if ((unsigned)ch >= (unsigned)g.h) continue;
      const float* row = in + plane + ch * g.w;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (v >= n) break;
        const int w0 = g.off + (j0 + v) * g.sx;
        for (int m = 0; m < g.size; ++m) {
          const int cw = w0 + m;
          if ((unsigned)cw < (unsigned)g.w) fold_tap<AVG>(f, v, row[cw], ch * g.w + cw);
        }
      }
    }
    fold_store<AVG>(f, n, r * g.outW + j0, plane, out, idx, vec != 0);
  }
}

// size 2, strides 2, off 0, W a multiple of 8, 16-byte aligned input: the 4
// outputs of a thread are the pairs of 8 contiguous floats of two rows, all
// columns in range (outW = W/2); only the second row can fall outside (odd H
// with padding 1)
template <bool AVG>
__global__ __launch_bounds__(256) void pool_fwd_2x2_kernel(int64_t planes, PoolGeom g,
                                                           const float* __restrict__ in,
                                                           float* __restrict__ out,
                                                           int64_t* __restrict__ idx, int vec) {
  const int qw = g.outW / V;
  const int64_t total = planes * g.outH * qw;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total;
       it += (int64_t)gridDim.x * blockDim.x) {
    const int j0 = (int)(it % qw) * V;
    const int64_t r = it / qw;
    const int i = (int)(r % g.outH);
    const int64_t plane = (r / g.outH) * g.h * g.w;
    Fold f;
    fold_init<AVG>(f);
#pragma unroll
    for (int kn = 0; kn < 2; ++kn) {
      const int ch = 2 * i + kn;
      if (ch >= g.h) break;
      const int at = ch * g.w + 2 * j0;
      const float4 a = *reinterpret_cast<const float4*>(in + plane + at);
      const float4 b = *reinterpret_cast<const float4*>(in + plane + at + 4);
      fold_tap<AVG>(f, 0, a.x, at);
      fold_tap<AVG>(f, 0, a.y, at + 1);
      fold_tap<AVG>(f, 1, a.z, at + 2);
      fold_tap<AVG>(f, 1, a.w, at + 3);
      fold_tap<AVG>(f, 2, b.x, at + 4);
      fold_tap<AVG>(f, 2, b.y, at + 5);
      fold_tap<AVG>(f, 3, b.z, at + 6);
      fold_tap<AVG>(f, 3, b.w, at + 7);
    }
    fold_store<AVG>(f, V, r * g.outW + j0, plane, out, idx, vec != 0);
  }
}

// sd = state.delta (the layer below's delta, the pool's input shape); VEC:
// W a multiple of 4 and sd 16-byte aligned
template <bool AVG, bool VEC>
__global__ __launch_bounds__(256) void pool_bwd_kernel(int64_t planes, PoolGeom g,
                                                       float* __restrict__ sd,
                                                       const int64_t* __restrict__ idx,
                                                       const float* __restrict__ delta) {
  const int qw = (g.w + V - 1) / V;
  const int64_t total = planes * g.h * qw;
  const float kk = (float)((int64_t)g.size * g.size);
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total;
       it += (int64_t)gridDim.x * blockDim.x) {
    const int x0 = (int)(it % qw) * V;
    const int64_t r = it / qw;  // input row (plane, y)
    const int y = (int)(r % g.h);
    // outputs covering row y: off + i*sy <= y <= off + i*sy + size - 1
    const int ny = y - g.off - g.size + 1;
    const int i_lo = ny > 0 ? (ny + g.sy - 1) / g.sy : 0;
    int i_hi = (y - g.off) / g.sy;
    if (i_hi > g.outH - 1) i_hi = g.outH - 1;
    if (i_lo > i_hi) continue;
    const int64_t oplane = (r / g.h) * g.outH * g.outW;
    const float* dp = delta + oplane;
    const int64_t* ip = AVG ? nullptr : idx + oplane;
    float* sdrow = sd + r * g.w;
    const int64_t base = r * g.w;  // absolute index of (plane, y, 0)
    const int n = g.w - x0 < V ? g.w - x0 : V;
    float acc[V];
    if constexpr (VEC) {
      const float4 t = *reinterpret_cast<const float4*>(sdrow + x0);
      acc[0] = t.x, acc[1] = t.y, acc[2] = t.z, acc[3] = t.w;
    } else {
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = v < n ? sdrow[x0 + v] : 0.0f;
    }
    unsigned hit = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (v >= n) break;
      const int x = x0 + v;
      const int nx = x - g.off - g.size + 1;
      const int j_lo = nx > 0 ? (nx + g.sx - 1) / g.sx : 0;
      int j_hi = (x - g.off) / g.sx;
      if (j_hi > g.outW - 1) j_hi = g.outW - 1;
      for (int i = i_lo; i <= i_hi; ++i)
        for (int j = j_lo; j <= j_hi; ++j) {
          const int o = i * g.outW + j;
          if constexpr (AVG) {
            acc[v] = acc[v] + dp[o] / kk;
            hit |= 1u << v;
          } else if (ip[o] == base + x) {
            acc[v] = acc[v] + dp[o];
            hit |= 1u << v;
          }
        }
    }
    if (!hit) continue;
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(sdrow + x0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
      for (int v = 0; v < V; ++v)
        if (hit >> v & 1u) sdrow[x0 + v] = acc[v];
    }
  }
}

int blocks_for(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool AVG>
hipError_t forward(int64_t planes, const PoolGeom& g, const float* in, float* out, int64_t* idx,
                   hipStream_t s) {
  if (planes * g.outH * g.outW <= 0) return hipSuccess;
  const int vec = g.outW % V == 0 && aligned16(out) && (AVG || !idx || aligned16(idx));
  const int64_t items = planes * g.outH * ((g.outW + V - 1) / V);
  if (g.size == 2 && g.sx == 2 && g.sy == 2 && g.off == 0 && g.w % 8 == 0 &&
      g.outW == g.w / 2 && aligned16(in))
    hipLaunchKernelGGL(pool_fwd_2x2_kernel<AVG>, dim3(blocks_for(items)), dim3(256), 0, s, planes,
                       g, in, out, idx, vec);
  else
    hipLaunchKernelGGL(pool_fwd_kernel<AVG>, dim3(blocks_for(items)), dim3(256), 0, s, planes, g,
                       in, out, idx, vec);
  return hipGetLastError();
}

template <bool AVG>
hipError_t backward(int64_t planes, const PoolGeom& g, float* sd, const int64_t* idx,
                    const float* delta, hipStream_t s) {
  if (planes * g.outH * g.outW <= 0 || planes * g.h * g.w <= 0) return hipSuccess;
  const int64_t items = planes * g.h * ((g.w + V - 1) / V);
  if (g.w % V == 0 && aligned16(sd))
    hipLaunchKernelGGL((pool_bwd_kernel<AVG, true>), dim3(blocks_for(items)), dim3(256), 0, s,
                       planes, g, sd, idx, delta);
  else
    hipLaunchKernelGGL((pool_bwd_kernel<AVG, false>), dim3(blocks_for(items)), dim3(256), 0, s,
                       planes, g, sd, idx, delta);
  return hipGetLastError();
}

// ---- global average pool (TAvgPoolLayer, navgpoollayer.pas:60-108) ---------
// The data is [planes][n], planes contiguous.  Forward: out[p] = Sum(plane p)
// / float(n), Sum in vssum_avx2's order (ntensors.pas:3592-3620; vssum8 in
// batchnorm.hip is the one-thread form).  Eight lanes own a plane, lane j
// being accumulator j: from +0 it adds elements j, j+8, j+16, ... of the
// first 8*(n div 8); the fold a_j + a_(j+4) and the two pair adds (s0+s1) +
// (s2+s3) run across the lanes; lane 0 then adds the n mod 8 tail elements in
// index order and divides once.  A wave64 holds eight planes, a block 32.
// n is the same for every lane, so every loop trip count is wave-uniform and
// the cross-lane steps run converged; a lane whose plane is past the end
// reads the last plane and only its store is masked.
constexpr int GAP_PLANES = 256 / 8;   // planes per block
constexpr int GAP_MAX_BLOCKS = 2048;  // 8 resident blocks on each of 256 CUs; beyond: more trips

__global__ __launch_bounds__(256) void global_avgpool_fwd_kernel(int64_t planes, int64_t n,
                                                                 const float* __restrict__ in,
                                                                 float* __restrict__ out) {
  const int l = threadIdx.x & 7;
  const int64_t nblk = n >> 3;
  const int64_t nb8 = nblk << 3;
  const int tail = (int)(n - nb8);
  const float fn = (float)n;  // exact: n <= 2^24
  const int64_t groups = (planes + GAP_PLANES - 1) / GAP_PLANES;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t plane = g * GAP_PLANES + (threadIdx.x >> 3);
    const bool live = plane < planes;
    const float* a = in + (live ? plane : planes - 1) * n;
    float acc = 0.0f;
    int64_t b = 0;
    for (; b + 4 <= nblk; b += 4) {  // four loads ahead of the lane's adds
      const float w0 = a[8 * b + l], w1 = a[8 * b + 8 + l], w2 = a[8 * b + 16 + l],
                  w3 = a[8 * b + 24 + l];
      acc = acc + w0;
      acc = acc + w1;
      acc = acc + w2;
      acc = acc + w3;
    }
    for (; b < nblk; ++b) acc = acc + a[8 * b + l];
    const float s = acc + __shfl_down(acc, 4, 8);  // lanes 0..3: a_j + a_(j+4)
    const float h = s + __shfl_down(s, 1, 8);      // lane 0: s0+s1, lane 2: s2+s3
    float r = h + __shfl_down(h, 2, 8);            // lane 0: (s0+s1) + (s2+s3)
    if (tail) {
      const float tv = l < tail ? a[nb8 + l] : 0.0f;
      for (int k = 0; k < tail; ++k) r = r + __shfl(tv, k, 8);
    }
    if (live && l == 0) out[plane] = r / fn;
  }
}

// Backward: state_delta[p*n + i] += delta[p] / float(n), the quotient rounded
// once (TTensor.Add of a scalar), then one add per element.  The buffer is
// walked flat: `head` elements up to the first 16-byte boundary and the
// elements after the last whole group one thread each, float4 groups between;
// a group may span planes (any n, 1 included), so the plane and its quotient
// advance inside it.  narrow: total < 2^32, the element's plane by a 32-bit
// division.
__global__ __launch_bounds__(256) void global_avgpool_bwd_kernel(int64_t total, int64_t n,
                                                                 int64_t head, int64_t nvec,
                                                                 int narrow,
                                                                 const float* __restrict__ delta,
                                                                 float* __restrict__ sd) {
  const float fn = (float)n;
  const int64_t items = nvec + (total - 4 * nvec);
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items;
       it += (int64_t)gridDim.x * blockDim.x) {
    const bool vec = it < nvec;
    // scalar items: the head elements first, then those after the groups
    const int64_t k = it - nvec;
    const int64_t e = vec ? head + 4 * it : (k < head ? k : 4 * nvec + k);
    int64_t p = narrow ? (int64_t)((uint32_t)e / (uint32_t)n) : e / n;
    if (!vec) {
      sd[e] = sd[e] + delta[p] / fn;
      continue;
    }
    int64_t r = e - p * n;
    float q = delta[p] / fn;
    float4 t = *reinterpret_cast<float4*>(sd + e);
    float x[V] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (r == n) {
        r = 0;
        q = delta[++p] / fn;
      }
      x[v] = x[v] + q;
      ++r;
    }
    *reinterpret_cast<float4*>(sd + e) = make_float4(x[0], x[1], x[2], x[3]);
  }
}

}  // namespace

hipError_t launch_global_avgpool_forward(int64_t planes, int64_t n, const float* in, float* out,
                                         hipStream_t s) {
  const int64_t groups = (planes + GAP_PLANES - 1) / GAP_PLANES;
  const int blocks = (int)(groups < GAP_MAX_BLOCKS ? groups : GAP_MAX_BLOCKS);
  hipLaunchKernelGGL(global_avgpool_fwd_kernel, dim3(blocks), dim3(256), 0, s, planes, n, in, out);
  return hipGetLastError();
}

hipError_t launch_global_avgpool_backward(int64_t planes, int64_t n, const float* delta,
                                          float* state_delta, hipStream_t s) {
  const int64_t total = planes * n;
  int64_t head = (4 - (int64_t)((reinterpret_cast<uintptr_t>(state_delta) >> 2) & 3)) & 3;
  if (head > total) head = total;
  const int64_t nvec = (total - head) / V;
  const int64_t items = nvec + (total - V * nvec);
  int64_t blocks = (items + 255) / 256;
  if (blocks > GAP_MAX_BLOCKS) blocks = GAP_MAX_BLOCKS;
  hipLaunchKernelGGL(global_avgpool_bwd_kernel, dim3((int)blocks), dim3(256), 0, s, total, n, head,
                     nvec, total < (int64_t)1 << 32 ? 1 : 0, delta, state_delta);
  return hipGetLastError();
}

hipError_t launch_maxpool_forward(int64_t planes, const PoolGeom& g, const float* in, float* out,
                                  int64_t* indexes, hipStream_t s) {
  return forward<false>(planes, g, in, out, indexes, s);
}
hipError_t launch_avgpool_forward(int64_t planes, const PoolGeom& g, const float* in, float* out,
                                  hipStream_t s) {
  return forward<true>(planes, g, in, out, nullptr, s);
}
hipError_t launch_maxpool_backward(int64_t planes, const PoolGeom& g, float* state_delta,
                                   const int64_t* indexes, const float* delta, hipStream_t s) {
  return backward<false>(planes, g, state_delta, indexes, delta, s);
}
hipError_t launch_avgpool_backward(int64_t planes, const PoolGeom& g, float* state_delta,
                                   const float* delta, hipStream_t s) {
  return backward<true>(planes, g, state_delta, nullptr, delta, s);
}

}  // namespace tns
