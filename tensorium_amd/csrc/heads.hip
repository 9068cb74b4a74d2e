// heads.hip — dropout and the elementwise loss heads of a classifier:
// forward_dropout / backward_dropout / cost_l2 (the reference's device
// kernels, cuda_sgemm.cu:1617-1662) and the logistic cross entropy
// (TLogisticLayer.logisticCrossEntropy, nlogisticlayer.pas:67-78, the CPU
// statement, as xent_softmax_k takes the softmax one).
//
// Dropout's random number is a pure function of (seed, i): one xorshift64*
// step of x = seed + i (seed a 32-bit unsigned value, the sum in 64 bits),
// r = x mod 2^28, rnd = float(r) / 2^28.  Only bits 0..27 of the product
// are kept; they are those of the low 32 bits of the shifted x times the
// low 32 bits of the multiplier, so one 32-bit multiply gives them.  The
// conversion rounds to nearest even (r has up to 28 bits) and the division
// by 2^28 is an exact multiply by 2^-28 (no result is subnormal).
//   dst = rnd < probability ? +0.0f : src * scale
// A dropped element is +0.0f whatever src held; a kept one is one rounded
// multiply.  The backward is the same select over the stored rnd.
//
// Shape: 256 threads, a thread owns 4 adjacent elements: 16-byte loads and
// stores when every pointer of the call is 16-byte aligned, scalar otherwise
// and in the tail.  A thread reads its elements before it writes them, so
// src == dst (the reference's call, ndropoutlayer.pas:162, 170) is safe;
// src and dst therefore carry no __restrict__.  int64 indexing, grid-stride.
#include "tns_internal.hpp"

namespace tns {
namespace {

constexpr int V = 4;
constexpr float SEPS = 0.000001f;  // sEPSILON, ntensors.pas:95

__device__ __forceinline__ float dropout_rnd(uint64_t x) {
  x ^= x >> 12;
  x ^= x << 25;
  x ^= x >> 27;
  const uint32_t r = ((uint32_t)x * 0x4F6CDD1Du) & 0x0FFFFFFFu;
  return (float)r * 0x1p-28f;
}

struct DropFwd {
  uint64_t seed;
  float prob, scale;
  const float* src;
  float* __restrict__ rnd;
  float* dst;
  __device__ __forceinline__ void vec(int64_t i) const {
    const float4 s = *reinterpret_cast<const float4*>(src + i);
    const float in[V] = {s.x, s.y, s.z, s.w};
    float r[V], o[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      r[v] = dropout_rnd(seed + (uint64_t)(i + v));
      o[v] = r[v] < prob ? 0.0f : in[v] * scale;
    }
    *reinterpret_cast<float4*>(rnd + i) = make_float4(r[0], r[1], r[2], r[3]);
    *reinterpret_cast<float4*>(dst + i) = make_float4(o[0], o[1], o[2], o[3]);
  }
  __device__ __forceinline__ void one(int64_t i) const {
    const float s = src[i];
    const float r = dropout_rnd(seed + (uint64_t)i);
    rnd[i] = r;
    dst[i] = r < prob ? 0.0f : s * scale;
  }
};

struct DropBwd {
  float prob, scale;
  const float* src;
  const float* __restrict__ rnd;
  float* dst;
  __device__ __forceinline__ void vec(int64_t i) const {
    const float4 s = *reinterpret_cast<const float4*>(src + i);
    const float4 r = *reinterpret_cast<const float4*>(rnd + i);
    *reinterpret_cast<float4*>(dst + i) =
        make_float4(r.x < prob ? 0.0f : s.x * scale, r.y < prob ? 0.0f : s.y * scale,
                    r.z < prob ? 0.0f : s.z * scale, r.w < prob ? 0.0f : s.w * scale);
  }
  __device__ __forceinline__ void one(int64_t i) const {
    const float s = src[i];
    dst[i] = rnd[i] < prob ? 0.0f : s * scale;
  }
};

// r = truth - pred; delta = r; error = r * r, each one rounding
struct CostL2 {
  const float* __restrict__ pred;
  const float* __restrict__ truth;
  float* __restrict__ delta;
  float* __restrict__ error;
  __device__ __forceinline__ void vec(int64_t i) const {
    const float4 p = *reinterpret_cast<const float4*>(pred + i);
    const float4 t = *reinterpret_cast<const float4*>(truth + i);
    const float4 r = make_float4(t.x - p.x, t.y - p.y, t.z - p.z, t.w - p.w);
    *reinterpret_cast<float4*>(delta + i) = r;
    *reinterpret_cast<float4*>(error + i) = make_float4(r.x * r.x, r.y * r.y, r.z * r.z, r.w * r.w);
  }
  __device__ __forceinline__ void one(int64_t i) const {
    const float r = truth[i] - pred[i];
    delta[i] = r;
    error[i] = r * r;
  }
};

// error = -t*ln(max(p, eps)) - (1-t)*ln(max(1-p, eps)): max (Pascal's: a > b
// ? a : b), 1-p and 1-t in float, ln in double, the two products and the
// subtraction in double, one rounding to float (FPC: single operands, ln
// returns double)
__device__ __forceinline__ float logistic_xent(float t, float p) {
  const float a = p > SEPS ? p : SEPS;
  const float q = 1.0f - p;
  const float b = q > SEPS ? q : SEPS;
  const float u = 1.0f - t;
  return (float)((double)(-t) * log((double)a) - (double)u * log((double)b));
}

struct XentLogistic {
  const float* __restrict__ pred;
  const float* __restrict__ truth;
  float* __restrict__ delta;
  float* __restrict__ error;
  __device__ __forceinline__ void vec(int64_t i) const {
    const float4 p = *reinterpret_cast<const float4*>(pred + i);
    const float4 t = *reinterpret_cast<const float4*>(truth + i);
    *reinterpret_cast<float4*>(delta + i) = make_float4(t.x - p.x, t.y - p.y, t.z - p.z, t.w - p.w);
    *reinterpret_cast<float4*>(error + i) =
        make_float4(logistic_xent(t.x, p.x), logistic_xent(t.y, p.y), logistic_xent(t.z, p.z),
                    logistic_xent(t.w, p.w));
  }
  __device__ __forceinline__ void one(int64_t i) const {
    const float t = truth[i], p = pred[i];
    delta[i] = t - p;
    error[i] = logistic_xent(t, p);
  }
};

// item `it` = elements [4*it, 4*it + 4) clipped to n
template <class Op, bool VEC>
__global__ __launch_bounds__(256) void heads_kernel(int64_t n, Op op) {
  const int64_t items = (n + V - 1) / V;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items;
       it += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = it * V;
    if (VEC && i0 + V <= n) {
      op.vec(i0);
    } else {
      const int m = n - i0 < V ? (int)(n - i0) : V;
      // (dropout in place: element i is read and written by this thread
      // only, each element on its own)
      for (int v = 0; v < m; ++v) op.one(i0 + v);
    }
  }
}

bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t a = 0;
  for (const void* p : ps) a |= reinterpret_cast<uintptr_t>(p);
  return (a & 15) == 0;
}

template <class Op>
hipError_t launch(int64_t n, const Op& op, bool vec, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  int64_t b = ((n + V - 1) / V + 255) / 256;
  const dim3 grid((unsigned)(b > 16384 ? 16384 : b));
  if (vec)
    hipLaunchKernelGGL((heads_kernel<Op, true>), grid, dim3(256), 0, s, n, op);
  else
    hipLaunchKernelGGL((heads_kernel<Op, false>), grid, dim3(256), 0, s, n, op);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_dropout_forward(int64_t n, uint32_t seed, float probability, float scale,
                                  const float* src, float* rnd, float* dst, hipStream_t s) {
  return launch(n, DropFwd{seed, probability, scale, src, rnd, dst}, aligned16({src, rnd, dst}), s);
}
hipError_t launch_dropout_backward(int64_t n, float probability, float scale, const float* src,
                                   const float* rnd, float* dst, hipStream_t s) {
  return launch(n, DropBwd{probability, scale, src, rnd, dst}, aligned16({src, rnd, dst}), s);
}
hipError_t launch_cost_l2(int64_t n, const float* pred, const float* truth, float* delta,
                          float* error, hipStream_t s) {
  return launch(n, CostL2{pred, truth, delta, error}, aligned16({pred, truth, delta, error}), s);
}
hipError_t launch_xent_logistic(int64_t n, const float* pred, const float* truth, float* delta,
                                float* error, hipStream_t s) {
  return launch(n, XentLogistic{pred, truth, delta, error},
                aligned16({pred, truth, delta, error}), s);
}

}  // namespace tns
