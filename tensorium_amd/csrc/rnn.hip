// rnn.hip — the elementwise stage of one RNN time step, fused: what
// TRNNLayer.rnnStepForward / rnnStepBackward (nrnnlayer.pas:148-216) and the
// head of TConnectedLayer.forward / backward (nconnectedlayer.pas:157-322)
// issue around the three connected sub-layers (input, self, output) as
// forwardBias x2, ActivateArray x2, fill / copy, addvv x2 and as clamp +
// DeriveArray (+ copy + clamp + DeriveArray), as one kernel per direction.
// Every written operation is one float32 rounding (the file is compiled
// without contraction); activations and gradients are tns_act.hpp's.
//
// State forward, per element k (bias column k % H; a null bias: the slice is
// normalized and biased already, the batch-norm case):
//   a = in_slice[k];    a = a + in_bias[k % H];    a = act(a, in_act)
//   b = self_slice[k];  b = b + self_bias[k % H];  b = act(b, self_act)
//   s = (state_prev ? state_prev[k] : 0.0f) + a;   s = s + b
//   a -> in_slice[k];  b -> self_slice[k];  s -> state_next[k]
// The sum is the reference's fill (or copy) and two adds, two roundings:
// 0.0f + a is written out, so a = b = -0 gives +0 as there.
//
// Delta backward, per element k:
//   d = clamp1(delta[k]) * grad(out[k], act)     -> delta[k]
//   delta2[k] = clamp1(d) * grad(out2[k], act2)  (delta2 not null)
// clamp1 is clamp_kernel's form (v < -1 ? -1 : v > 1 ? 1 : v), which keeps a
// NaN.
//
// Shape (lstm.hip's): 256 threads, a thread owns 4 adjacent elements; 16-byte
// accesses when every slice pointer of the call is 16-byte aligned (the biases
// are read one column at a time), scalar otherwise (a step's slice starts at
// step*streams*hidden floats, so the scalar path is an ordinary one) and in
// the tail.  A group of 4 may straddle a row end when H % 4 != 0: the column
// is carried per element.  A thread reads all of its elements' operands before
// it writes any of them, so the in-place operands (in_slice, self_slice,
// delta, and state_prev == state_next) are safe and carry no __restrict__.
// int64 indexing.
#include "tns_act.hpp"
#include "tns_internal.hpp"

namespace tns {
namespace {

constexpr int V = 4;

__device__ __forceinline__ float clamp1(float v) {
  return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
}

struct StateFwd {
  int64_t H;
  float* in_slice;
  const float* __restrict__ in_bias;  // may be null
  int in_act;
  float* self_slice;
  const float* __restrict__ self_bias;  // may be null
  int self_act;
  const float* state_prev;  // may be null, may be state_next
  float* state_next;

  // col = k % H
  __device__ __forceinline__ void step(float& a, float& b, float prev, int64_t col,
                                       float& s) const {
    if (in_bias) a = a + in_bias[col];
    a = act_apply(a, in_act);
    if (self_bias) b = b + self_bias[col];
    b = act_apply(b, self_act);
    s = prev + a;
    s = s + b;
  }
  __device__ __forceinline__ void vec(int64_t k) const {
    const float4 a4 = *reinterpret_cast<const float4*>(in_slice + k);
    const float4 b4 = *reinterpret_cast<const float4*>(self_slice + k);
    float4 p4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (state_prev) p4 = *reinterpret_cast<const float4*>(state_prev + k);
    float a[V] = {a4.x, a4.y, a4.z, a4.w}, b[V] = {b4.x, b4.y, b4.z, b4.w};
    const float p[V] = {p4.x, p4.y, p4.z, p4.w};
    float s[V];
    int64_t col = k % H;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      step(a[v], b[v], p[v], col, s[v]);
      if (++col == H) col = 0;
    }
    *reinterpret_cast<float4*>(in_slice + k) = make_float4(a[0], a[1], a[2], a[3]);
    *reinterpret_cast<float4*>(self_slice + k) = make_float4(b[0], b[1], b[2], b[3]);
    *reinterpret_cast<float4*>(state_next + k) = make_float4(s[0], s[1], s[2], s[3]);
  }
  __device__ __forceinline__ void one(int64_t k) const {
    float a = in_slice[k], b = self_slice[k], s;
    const float p = state_prev ? state_prev[k] : 0.0f;
    step(a, b, p, k % H, s);
    in_slice[k] = a;
    self_slice[k] = b;
    state_next[k] = s;
  }
};

struct DeltaBwd {
  float* delta;
  const float* __restrict__ out;
  int act;
  float* __restrict__ delta2;  // may be null
  const float* __restrict__ out2;
  int act2;

  __device__ __forceinline__ void vec(int64_t k) const {
    const float4 d4 = *reinterpret_cast<const float4*>(delta + k);
    const float4 o4 = *reinterpret_cast<const float4*>(out + k);
    const float d[V] = {d4.x, d4.y, d4.z, d4.w}, o[V] = {o4.x, o4.y, o4.z, o4.w};
    float r[V];
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = clamp1(d[v]) * grad_apply(o[v], act);
    if (delta2) {
      const float4 q4 = *reinterpret_cast<const float4*>(out2 + k);
      const float q[V] = {q4.x, q4.y, q4.z, q4.w};
      float r2[V];
#pragma unroll
      for (int v = 0; v < V; ++v) r2[v] = clamp1(r[v]) * grad_apply(q[v], act2);
      *reinterpret_cast<float4*>(delta2 + k) = make_float4(r2[0], r2[1], r2[2], r2[3]);
    }
    *reinterpret_cast<float4*>(delta + k) = make_float4(r[0], r[1], r[2], r[3]);
  }
  __device__ __forceinline__ void one(int64_t k) const {
    const float d = clamp1(delta[k]) * grad_apply(out[k], act);
    if (delta2) {
      const float q = out2[k];
      delta2[k] = clamp1(d) * grad_apply(q, act2);
    }
    delta[k] = d;
  }
};

// item `it` = elements [4*it, 4*it + 4) clipped to n
template <class Op, bool VEC>
__global__ __launch_bounds__(256) void rnn_step_kernel(int64_t n, Op op) {
  const int64_t items = (n + V - 1) / V;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items;
       it += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = it * V;
    if (VEC && i0 + V <= n) {
      op.vec(i0);
    } else {
      const int m = n - i0 < V ? (int)(n - i0) : V;
      // (in place: element k is read and written by this thread only, each
      // element on its own)
      for (int v = 0; v < m; ++v) op.one(i0 + v);
    }
  }
}

bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t a = 0;
  for (const void* p : ps) a |= reinterpret_cast<uintptr_t>(p);  // (null adds nothing)
  return (a & 15) == 0;
}

template <class Op>
hipError_t launch(int64_t n, const Op& op, bool vec, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  int64_t b = ((n + V - 1) / V + 255) / 256;
  const dim3 grid((unsigned)(b > 16384 ? 16384 : b));
  if (vec)
    hipLaunchKernelGGL((rnn_step_kernel<Op, true>), grid, dim3(256), 0, s, n, op);
  else
    hipLaunchKernelGGL((rnn_step_kernel<Op, false>), grid, dim3(256), 0, s, n, op);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_rnn_state_forward(int64_t n, int64_t H, float* in_slice, const float* in_bias,
                                    int in_act, float* self_slice, const float* self_bias,
                                    int self_act, const float* state_prev, float* state_next,
                                    hipStream_t s) {
  return launch(n,
                StateFwd{H, in_slice, in_bias, in_act, self_slice, self_bias, self_act,
                         state_prev, state_next},
                aligned16({in_slice, self_slice, state_prev, state_next}), s);
}

hipError_t launch_rnn_delta_backward(int64_t n, float* delta, const float* out, int act,
                                     float* delta2, const float* out2, int act2, hipStream_t s) {
  return launch(n, DeltaBwd{delta, out, act, delta2, out2, act2},
                aligned16({delta, out, delta2, delta2 ? out2 : nullptr}), s);
}

}  // namespace tns
