// lstm.hip — the gate stage of one LSTM time step, fused: what
// TLSTMLayer.forwardGPU / backwardGPU (nlstmlayer.pas:933-973, 1046-1255)
// issue as ~16 / ~30 elementwise launches (addvv, ActivateArray, mulvv,
// fmavv, copy, DeriveArray) around the eight connected sub-layers, as one
// kernel per direction.  Every written operation is one float32 rounding (the
// file is compiled without contraction), the activations are tns_act.hpp's:
// logistic = 1/(1+exp(-x)) in double rounded once, tanh = (px-nx)/(px+nx) on
// the single-rounded exponentials, gradients (1-y)*y and 1-y*y.
//
// Forward, per element k (a_x = w_x[k] + u_x[k], one rounded add):
//   f = logistic(a_f)  i = logistic(a_i)  g = tanh(a_g)  o = logistic(a_o)
//   t = i*g;  c = c*f;  c = c + t;  h = tanh(c)*o
//   c -> c_state[k], cell_slice[k];  h -> h_state[k], out_slice[k]
// Backward, per element k:
//   t = tanh(cell_i[k]);  d = delta_i[k]
//   e = d*o;  e = e*(1 - t*t);  e = dc[k] + e
//   do = (d*t)*((1-o)*o)   dg = (e*i)*(1 - g*g)
//   di = (e*g)*((1-i)*i)   df = (e*cprev[k])*((1-f)*f)
//   dc[k] = e*f
// tanh(cell) is evaluated once (the call sequence evaluates it twice, to the
// same value).  The four gate deltas are stored clamped to [-1, 1] — the
// first thing the sub-layer's backward does to them (cuda.clamp(delta, 1),
// nconnectedlayer.pas:771), in clamp_kernel's form, which keeps a NaN — to
// the w-side slice and, where given, to the u-side slice.  dc is not clamped.
//
// Shape (heads.hip's): 256 threads, a thread owns 4 adjacent elements; 16-byte
// accesses when every pointer of the call is 16-byte aligned, scalar
// otherwise (a step's slice starts at step*streams*outputs floats, so the
// scalar path is an ordinary one) and in the tail.  A thread reads all of its
// elements' operands before it writes any of them, so the in-place operands
// (c_state, dc) are safe and carry no __restrict__.  int64 indexing.
#include "tns_act.hpp"
#include "tns_internal.hpp"

namespace tns {
namespace {

constexpr int V = 4;
constexpr int LOGISTIC = 0, TANH = 6;  // TActivationType ordinals

__device__ __forceinline__ float clamp1(float v) {
  return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
}

struct Gates {
  float f, i, g, o;
};

struct Pre {
  const float* __restrict__ wf;
  const float* __restrict__ wi;
  const float* __restrict__ wg;
  const float* __restrict__ wo;
  const float* __restrict__ uf;
  const float* __restrict__ ui;
  const float* __restrict__ ug;
  const float* __restrict__ uo;
  __device__ __forceinline__ Gates one(int64_t k) const {
    return Gates{act_apply(wf[k] + uf[k], LOGISTIC), act_apply(wi[k] + ui[k], LOGISTIC),
                 act_apply(wg[k] + ug[k], TANH), act_apply(wo[k] + uo[k], LOGISTIC)};
  }
  __device__ __forceinline__ void vec(int64_t k, Gates* q) const {
    const float4 a = *reinterpret_cast<const float4*>(wf + k);
    const float4 b = *reinterpret_cast<const float4*>(uf + k);
    const float4 c = *reinterpret_cast<const float4*>(wi + k);
    const float4 d = *reinterpret_cast<const float4*>(ui + k);
    const float4 e = *reinterpret_cast<const float4*>(wg + k);
    const float4 f = *reinterpret_cast<const float4*>(ug + k);
    const float4 g = *reinterpret_cast<const float4*>(wo + k);
    const float4 h = *reinterpret_cast<const float4*>(uo + k);
    const float af[V] = {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
    const float ai[V] = {c.x + d.x, c.y + d.y, c.z + d.z, c.w + d.w};
    const float ag[V] = {e.x + f.x, e.y + f.y, e.z + f.z, e.w + f.w};
    const float ao[V] = {g.x + h.x, g.y + h.y, g.z + h.z, g.w + h.w};
#pragma unroll
    for (int v = 0; v < V; ++v)
      q[v] = Gates{act_apply(af[v], LOGISTIC), act_apply(ai[v], LOGISTIC), act_apply(ag[v], TANH),
                   act_apply(ao[v], LOGISTIC)};
  }
};

struct GatesFwd {
  Pre pre;
  float* c_state;
  float* __restrict__ h_state;
  float* __restrict__ cell;
  float* __restrict__ out;
  static __device__ __forceinline__ void step(const Gates& q, float c0, float& c, float& h) {
    const float t = q.i * q.g;
    c = c0 * q.f;
    c = c + t;
    h = act_apply(c, TANH) * q.o;
  }
  __device__ __forceinline__ void vec(int64_t k) const {
    Gates q[V];
    pre.vec(k, q);
    const float4 c4 = *reinterpret_cast<const float4*>(c_state + k);
    const float c0[V] = {c4.x, c4.y, c4.z, c4.w};
    float c[V], h[V];
#pragma unroll
    for (int v = 0; v < V; ++v) step(q[v], c0[v], c[v], h[v]);
    const float4 cv = make_float4(c[0], c[1], c[2], c[3]);
    const float4 hv = make_float4(h[0], h[1], h[2], h[3]);
    *reinterpret_cast<float4*>(c_state + k) = cv;
    *reinterpret_cast<float4*>(cell + k) = cv;
    *reinterpret_cast<float4*>(h_state + k) = hv;
    *reinterpret_cast<float4*>(out + k) = hv;
  }
  __device__ __forceinline__ void one(int64_t k) const {
    const Gates q = pre.one(k);
    float c, h;
    step(q, c_state[k], c, h);
    c_state[k] = c;
    cell[k] = c;
    h_state[k] = h;
    out[k] = h;
  }
};

struct GateDeltas {
  float df, di, dg, dO, dc;
};

struct GatesBwd {
  Pre pre;
  const float* __restrict__ cell_i;
  const float* __restrict__ cprev;
  const float* __restrict__ delta_i;
  float* dc;
  float* __restrict__ dwf;
  float* __restrict__ dwi;
  float* __restrict__ dwg;
  float* __restrict__ dwo;
  float* __restrict__ duf;  // the u-side slices: each may be null
  float* __restrict__ dui;
  float* __restrict__ dug;
  float* __restrict__ duo;
  static __device__ __forceinline__ GateDeltas step(const Gates& q, float cell, float cp, float d,
                                                    float dc0) {
    const float t = act_apply(cell, TANH);
    float e = d * q.o;
    e = e * grad_apply(t, TANH);
    e = dc0 + e;
    GateDeltas r;
    r.dO = clamp1((d * t) * grad_apply(q.o, LOGISTIC));
    r.dg = clamp1((e * q.i) * grad_apply(q.g, TANH));
    r.di = clamp1((e * q.g) * grad_apply(q.i, LOGISTIC));
    r.df = clamp1((e * cp) * grad_apply(q.f, LOGISTIC));
    r.dc = e * q.f;
    return r;
  }
  static __device__ __forceinline__ void put4(float* w, float* u, int64_t k, const float4& v) {
    *reinterpret_cast<float4*>(w + k) = v;
    if (u) *reinterpret_cast<float4*>(u + k) = v;
  }
  static __device__ __forceinline__ void put1(float* w, float* u, int64_t k, float v) {
    w[k] = v;
    if (u) u[k] = v;
  }
  __device__ __forceinline__ void vec(int64_t k) const {
    Gates q[V];
    pre.vec(k, q);
    const float4 a = *reinterpret_cast<const float4*>(cell_i + k);
    const float4 b = *reinterpret_cast<const float4*>(cprev + k);
    const float4 c = *reinterpret_cast<const float4*>(delta_i + k);
    const float4 d = *reinterpret_cast<const float4*>(dc + k);
    const float ce[V] = {a.x, a.y, a.z, a.w}, cp[V] = {b.x, b.y, b.z, b.w};
    const float de[V] = {c.x, c.y, c.z, c.w}, d0[V] = {d.x, d.y, d.z, d.w};
    GateDeltas r[V];
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = step(q[v], ce[v], cp[v], de[v], d0[v]);
    *reinterpret_cast<float4*>(dc + k) = make_float4(r[0].dc, r[1].dc, r[2].dc, r[3].dc);
    put4(dwo, duo, k, make_float4(r[0].dO, r[1].dO, r[2].dO, r[3].dO));
    put4(dwg, dug, k, make_float4(r[0].dg, r[1].dg, r[2].dg, r[3].dg));
    put4(dwi, dui, k, make_float4(r[0].di, r[1].di, r[2].di, r[3].di));
    put4(dwf, duf, k, make_float4(r[0].df, r[1].df, r[2].df, r[3].df));
  }
  __device__ __forceinline__ void one(int64_t k) const {
    const Gates q = pre.one(k);
    const GateDeltas r = step(q, cell_i[k], cprev[k], delta_i[k], dc[k]);
    dc[k] = r.dc;
    put1(dwo, duo, k, r.dO);
    put1(dwg, dug, k, r.dg);
    put1(dwi, dui, k, r.di);
    put1(dwf, duf, k, r.df);
  }
};

// item `it` = elements [4*it, 4*it + 4) clipped to n
template <class Op, bool VEC>
__global__ __launch_bounds__(256) void lstm_gates_kernel(int64_t n, Op op) {
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
    hipLaunchKernelGGL((lstm_gates_kernel<Op, true>), grid, dim3(256), 0, s, n, op);
  else
    hipLaunchKernelGGL((lstm_gates_kernel<Op, false>), grid, dim3(256), 0, s, n, op);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_lstm_gates_forward(int64_t n, const float* const w[4], const float* const u[4],
                                     float* c_state, float* h_state, float* cell_slice,
                                     float* out_slice, hipStream_t s) {
  const Pre pre{w[0], w[1], w[2], w[3], u[0], u[1], u[2], u[3]};
  return launch(n, GatesFwd{pre, c_state, h_state, cell_slice, out_slice},
                aligned16({w[0], w[1], w[2], w[3], u[0], u[1], u[2], u[3], c_state, h_state,
                           cell_slice, out_slice}),
                s);
}

hipError_t launch_lstm_gates_backward(int64_t n, const float* const w[4], const float* const u[4],
                                      const float* cell_i, const float* cprev,
                                      const float* delta_i, float* dc, float* const dw[4],
                                      float* const du[4], hipStream_t s) {
  const Pre pre{w[0], w[1], w[2], w[3], u[0], u[1], u[2], u[3]};
  return launch(n,
                GatesBwd{pre, cell_i, cprev, delta_i, dc, dw[0], dw[1], dw[2], dw[3], du[0],
                         du[1], du[2], du[3]},
                aligned16({w[0], w[1], w[2], w[3], u[0], u[1], u[2], u[3], cell_i, cprev, delta_i,
                           dc, dw[0], dw[1], dw[2], dw[3], du[0], du[1], du[2], du[3]}),
                s);
}

}  // namespace tns
