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

}  // namespace

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
