// tns_ctx.hpp — the context behind the C ABI's tns_ctx handle and the host
// helpers that tns_api.cpp and conv_api.cpp share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <initializer_list>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "tns_internal.hpp"

struct tns_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // device scratch, one buffer per SLOT_* below (im2col workspace, host-API
  // staging, dW partial sums, batch-norm block results, ...)
  static constexpr int kSlots = 12;
  float* scratch[kSlots] = {};
  size_t scratch_elems[kSlots] = {};
  // telemetry (TTensorMetrics-style, nopmetrics.pas:25-44)
  bool telemetry = false;
  double op_ms[TNS_OP_COUNT] = {0};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::mutex mu;  // serialises host-API use of one context
  // host-pointer pipeline: copy stream and per-chunk events
  hipStream_t copy_stream = nullptr;
  std::vector<hipEvent_t> pipe_ev;
  // conv backward: state.delta's chain (TN + col2im) runs on this side
  // stream while the dW product runs on `stream` (fork / join events)
  hipStream_t aux_stream = nullptr;
  // the joined overlap's side stream (TNS_OPT_BWD_OVERLAP = 1: state.delta's
  // chain beside the call's dW, joined before the call returns) at the
  // context stream's priority; aux_stream, the pipelined dW products' stream,
  // sits at the lowest
  hipStream_t ovl_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // TNS_OPT_BWD_OVERLAP = 2: dW products left running on aux_stream past the
  // call's return; the next call of any other entry point joins them first
  bool side_pending = false;
  hipStream_t home_stream = nullptr;  // the context's stream while `stream` is aux
  // the pending dW products' operand ranges: read (delta, input) and written
  // (weight_updates; the caller's workspace when the dW's im2col fills it).
  // A later call whose work on `stream` writes a read range, or touches a
  // written one, joins the side stream first; so does a call that takes a
  // scratch slot the side stream uses (side_slots)
  struct PendingDw {
    uintptr_t lo[2], hi[2];    // read by the dW
    uintptr_t wlo[2], whi[2];  // written by the dW
  };
  std::vector<PendingDw> pending;
  uint32_t side_slots = 0;
  // implicit-GEMM conv k-tables, one per (C, H, W, kH, kW, dY, dX)
  std::map<std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>, int*> ktabs;
};

namespace tns {

// every value tns_set_option sets (clamped there), and the two A/B switches
// read from the environment when the library loads
struct Options {
  int64_t strict_beta0 = 1;
  int64_t nt_sdot = 1;
  int64_t dx_fused = 1;
  // conv backward col = W^T . delta: -1 conv_tile4's k-major-A forms where
  // they apply, -2 the TN GEMM, v >= 0 form v (TNS_OPT_DX_TILE)
  int64_t dx_tile = -1;
  int64_t dx_conv = -1;
  int64_t dw_res = -1;
  // state.delta of the 1x1 / stride-1 layers on conv1x1.hip (W^T over the delta
  // planes, the col2im add in the epilogue) where conv1x1_pick takes the shape;
  // TNS_DX_C1=0 (A/B): the TN product / conv_dx forms
  bool dx_c1 = true;
  // the BN conv backward as one chain pass + normalizeDelta (launch_bn_backward_fused);
  // TNS_BN_FUSED=0 (A/B): the three-pass form
  bool bn_fused = true;
  // conv backward dW with the im2col matrix generated in the staging
  // (dw_tile.hip): -1 by measured shape, -2 never, v >= 0 form v (TNS_OPT_DW_TILE)
  int64_t dw_tile = -1;
  // conv backward: dW and state.delta concurrently on two streams (TNS_OPT_BWD_OVERLAP)
  int64_t bwd_overlap = 1;
  int64_t derive_sums = 0;
  // TNS_OPT_SCRATCH_CAP: largest context scratch buffer in floats (0 = none);
  // a larger request fails as an allocation failure would (tests reach the
  // fallback paths with it)
  int64_t scratch_cap = 0;
  int64_t tt_exact = 1;
  int64_t srss_quirk = 0;
  int64_t conv_variant = -1;
  int64_t conv_pad = -1;
};
extern Options g_opt;  // (tns_api.cpp)

enum { SLOT_COL = 0, SLOT_STAGE1 = 1, SLOT_STAGE2 = 2, SLOT_STAGE3 = 3, SLOT_DW = 4, SLOT_BN = 5,
       SLOT_MLP = 6, SLOT_WT = 7, SLOT_COL_DX = 8, SLOT_YOLO = 9, SLOT_RES_A = 10,
       SLOT_RES_B = 11, SLOT_COUNT = 12 };
static_assert(SLOT_COUNT == tns_ctx::kSlots, "one scratch buffer per slot");

inline int join_side(tns_ctx* c);

// scratch buffer `slot` of at least `elems` floats.  side: the caller is the
// pipelined conv backward taking a slot for the dW it queues behind the
// pending ones on the side stream (no join); any other caller of a slot the
// side stream still uses joins it first
inline int ensure_scratch(tns_ctx* c, int slot, int64_t elems, float** out, bool side = false) {
  if (elems < 1) elems = 1;
  if (!side && c->side_pending && (c->side_slots >> slot & 1u) && c->stream != c->aux_stream)
    if (int r = join_side(c)) return r;
  if (g_opt.scratch_cap > 0 && elems > g_opt.scratch_cap)
    return set_error(TNS_ERR_NOMEM, "scratch slot %d: %lld floats exceed the cap of %lld", slot,
                     (long long)elems, (long long)g_opt.scratch_cap);
  if ((size_t)elems > c->scratch_elems[slot]) {
    if (c->scratch[slot]) {
      hipStreamSynchronize(c->stream);
      if (c->aux_stream) hipStreamSynchronize(c->aux_stream);
      if (c->ovl_stream) hipStreamSynchronize(c->ovl_stream);
      if (c->home_stream) hipStreamSynchronize(c->home_stream);
      hipFree(c->scratch[slot]);
      c->scratch[slot] = nullptr;
      c->scratch_elems[slot] = 0;
    }
    hipError_t e = hipMalloc(&c->scratch[slot], (size_t)elems * sizeof(float));
    if (e != hipSuccess) {
      c->scratch[slot] = nullptr;
      // (clear HIP's sticky last error: the launch helpers report
      // hipGetLastError(), and a caller that falls back after this failure
      // must not see it on its first launch)
      hipGetLastError();
      return set_error(TNS_ERR_NOMEM, "hipMalloc(%lld floats) failed: %s", (long long)elems,
                       hipGetErrorString(e));
    }
    c->scratch_elems[slot] = (size_t)elems;
  }
  *out = c->scratch[slot];
  return TNS_OK;
}

// give a scratch buffer back (every stream that may still use it drained)
inline void release_scratch(tns_ctx* c, int slot) {
  if (!c->scratch[slot]) return;
  hipStreamSynchronize(c->stream);
  if (c->aux_stream) hipStreamSynchronize(c->aux_stream);
  if (c->ovl_stream) hipStreamSynchronize(c->ovl_stream);
  if (c->home_stream) hipStreamSynchronize(c->home_stream);
  hipFree(c->scratch[slot]);
  c->scratch[slot] = nullptr;
  c->scratch_elems[slot] = 0;
}

// the conv backward's side stream and its fork / join events, created
// together on the context's device; false (nothing kept) if any of them
// cannot be created, and the caller runs its sequential schedule
inline bool ensure_side_stream(tns_ctx* c) {
  if (c->aux_stream && c->ovl_stream && c->ev_fork && c->ev_join) return true;
  int prev = -1;
  hipGetDevice(&prev);
  // the pipelined dW products' stream (off the critical path) at the lowest
  // queue priority and the context's stream at the highest: the context's
  // work is dispatched first where both wait for CU room (YOLOv3 training
  // backward 17.96 -> 17.81 ms with the chain waves' issue priority,
  // batchnorm.hip; TNS_STREAM_PRIO=0 turns it off).  The joined overlap
  // waits for both halves of a call, so its stream keeps the default
  // priority (at the lowest, the joined conv backward lost 0.25 ms)
  int least = 0, greatest = 0;
  const char* sp = getenv("TNS_STREAM_PRIO");
  const bool prio = !(sp && sp[0] == '0') &&
                    hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
  bool ok = hipSetDevice(c->device) == hipSuccess &&
            (prio ? hipStreamCreateWithPriority(&c->aux_stream, hipStreamNonBlocking, least)
                  : hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking)) == hipSuccess &&
            hipStreamCreateWithFlags(&c->ovl_stream, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    if (c->aux_stream) hipStreamDestroy(c->aux_stream);
    if (c->ovl_stream) hipStreamDestroy(c->ovl_stream);
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    c->aux_stream = c->ovl_stream = nullptr;
    c->ev_fork = c->ev_join = nullptr;
    hipGetLastError();
  }
  if (prev >= 0) hipSetDevice(prev);
  return ok;
}

// the dW products a pipelined conv backward (TNS_OPT_BWD_OVERLAP = 2) left
// on the side stream: the context's stream waits for them from here on
inline int join_side(tns_ctx* c) {
  if (!c->side_pending) return TNS_OK;
  c->side_pending = false;
  c->pending.clear();
  c->side_slots = 0;
  hipError_t e = hipEventRecord(c->ev_join, c->aux_stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->ev_join, 0);
  if (e != hipSuccess) return set_error(TNS_ERR_HIP, "backward join: %s", hipGetErrorString(e));
  return TNS_OK;
}

struct OpTimer {
  tns_ctx* c;
  int op;
  explicit OpTimer(tns_ctx* c_, int op_) : c(c_), op(op_) {
    if (c->telemetry) hipEventRecord(c->ev0, c->stream);
  }
  ~OpTimer() {
    if (c->telemetry) {
      hipEventRecord(c->ev1, c->stream);
      hipEventSynchronize(c->ev1);
      float ms = 0.f;
      hipEventElapsedTime(&ms, c->ev0, c->ev1);
      c->op_ms[op] += ms;
    }
  }
};

// every entry point: the context exists, and earlier calls' side-stream work
// is ordered before whatever this call enqueues
inline int check_ctx(tns_ctx* c, bool join = true) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  return join ? join_side(c) : TNS_OK;
}

// an operand's extent: n elements every inc from p (empty when p is null or
// n <= 0).  A negative inc walks downward: p is the highest element touched.
// inc == 0 touches p alone and claims n elements (conservative)
struct Span {
  uintptr_t lo = 0, hi = 0;
};
inline Span span(const float* p, int64_t n, int64_t inc = 1) {
  Span s;
  if (!p || n <= 0) return s;
  if (inc < 0) {
    s.lo = (uintptr_t)(p + (n - 1) * inc);
    s.hi = (uintptr_t)(p + 1);
    return s;
  }
  s.lo = (uintptr_t)p;
  s.hi = (uintptr_t)(p + (n - 1) * (inc == 0 ? 1 : inc) + 1);
  return s;
}
// every non-conv entry point: the context exists, and — during a pipelined
// conv backward (TNS_OPT_BWD_OVERLAP = 2) — the side stream is joined only
// when this call's operands meet a pending dW's: it writes that dW's delta
// or input, or reads or writes its weight_updates / col workspace.  Calls
// that touch none of them (the shortcut's addvv between two conv layers, a
// route's copies, an upsample) leave the dW products running
inline int check_ops(tns_ctx* c, std::initializer_list<Span> writes,
                     std::initializer_list<Span> reads) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (!c->side_pending) return TNS_OK;
  auto meet = [](const Span& a, uintptr_t lo, uintptr_t hi) {
    return a.lo < a.hi && lo < hi && a.lo < hi && lo < a.hi;
  };
  for (const tns_ctx::PendingDw& d : c->pending)
    for (int y = 0; y < 2; ++y) {
      for (const Span& w : writes)
        if (meet(w, d.lo[y], d.hi[y]) || meet(w, d.wlo[y], d.whi[y])) return join_side(c);
      for (const Span& r : reads)
        if (meet(r, d.wlo[y], d.whi[y])) return join_side(c);
    }
  return TNS_OK;
}

inline int hip_status(hipError_t e, const char* what) {
  if (e != hipSuccess) return set_error(TNS_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  return TNS_OK;
}

inline int beta_mode_for(float beta) {
  if (beta == 1.0f) return BETA_ONE;
  if (beta == 0.0f && !g_opt.strict_beta0) return BETA_ZERO;
  return BETA_SCALE;
}

inline int do_gemm(tns_ctx* c, bool ta, bool tb, int64_t M, int64_t N, int64_t K, float alpha,
                   const float* A, int64_t lda, int64_t sA, const float* B, int64_t ldb, int64_t sB,
                   float beta, float* C, int64_t ldc, int64_t sC, int64_t batch, int epi,
                   const float* bias, int act, bool c_write_only = false, int variant = -1) {
  if (M < 0 || N < 0 || K < 0 || batch < 0)
    return set_error(TNS_ERR_ARG, "gemm: negative dimension");
  if (M == 0 || N == 0 || batch == 0) return TNS_OK;
  // leading dimensions, row-major (cblas_sgemm conventions)
  const int64_t minlda = ta ? M : K, minldb = tb ? K : N;
  if ((K > 0 && (lda < (minlda > 1 ? minlda : 1) || ldb < (minldb > 1 ? minldb : 1))) ||
      ldc < N)
    return set_error(TNS_ERR_ARG, "gemm: leading dimension too small (lda=%lld ldb=%lld ldc=%lld)",
                     (long long)lda, (long long)ldb, (long long)ldc);
  if (!C || (K > 0 && (!A || !B))) return set_error(TNS_ERR_ARG, "gemm: null operand");
  if (epi == EPI_BIAS_ACT && (!bias || !act_supported(act)))
    return set_error(TNS_ERR_ARG, "gemm: bad fused epilogue");
  GemmArgs a{};
  a.M = M; a.N = N; a.K = K;
  a.alpha = alpha; a.beta = beta;
  a.beta_mode = (c_write_only && beta == 0.0f) ? BETA_ZERO : beta_mode_for(beta);
  a.A = A; a.lda = lda; a.strideA = sA;
  a.B = B; a.ldb = ldb; a.strideB = sB;
  a.C = C; a.ldc = ldc; a.strideC = sC;
  a.batch = batch; a.epi = epi; a.bias = bias; a.act = act;
  OpTimer t(c, TNS_OP_GEMM);
  const GemmPlan p = plan_gemm(gemm_shape(a, ta, tb), variant, g_opt, get_sdot_form());
  // (a forced variant the plan refuses, or whose grid the launch refuses)
  const hipError_t e = launch_gemm_plan(p, a, c->stream);
  if ((p.err || e == hipErrorInvalidValue) && variant >= 0)
    return set_error(TNS_ERR_UNSUPPORTED, "gemm variant %d (%s) does not support this problem",
                     variant, sgemm_variant_name(variant));
  if (p.family == GEMM_TT) return hip_status(e, "sgemm_tt launch");
  if (p.family >= GEMM_NT_SDOT) return hip_status(e, "sgemm_nt launch");
  return hip_status(e, "sgemm launch");
}

inline ConvGeom geom(int64_t C, int64_t H, int64_t W, int64_t kH, int64_t kW, int64_t pH,
                     int64_t pW, int64_t sY, int64_t sX, int64_t dY, int64_t dX) {
  ConvGeom g;
  g.C = C; g.H = H; g.W = W; g.kH = kH; g.kW = kW; g.padH = pH; g.padW = pW;
  g.sY = sY; g.sX = sX; g.dY = dY; g.dX = dX;
  g.oh = out_dim(H, pH, kH, dY, sY);
  g.ow = out_dim(W, pW, kW, dX, sX);
  return g;
}

inline const char* geom_error(const ConvGeom& g) {
  if (g.C < 0 || g.H < 0 || g.W < 0 || g.kH <= 0 || g.kW <= 0 || g.sY <= 0 || g.sX <= 0 ||
      g.dY <= 0 || g.dX <= 0 || g.padH < 0 || g.padW < 0)
    return "im2col: invalid geometry";
  // kernel indexing is 32-bit inside one plane (image plane, col row) and
  // over the col rows; offsets of planes and rows are 64-bit
  if (g.C * g.kH * g.kW > 0x7fffffffLL || (g.oh > 0 ? g.oh : 1) * (g.ow > 0 ? g.ow : 1) >
      0x7fffffffLL || g.H * g.W > 0x7fffffffLL)
    return "im2col: image too large for 32-bit indexing";
  return nullptr;
}

inline int check_geom(const ConvGeom& g) {
  const char* m = geom_error(g);
  return m ? set_error(TNS_ERR_ARG, "%s", m) : TNS_OK;
}

// k-table of an implicit-GEMM convolution over Hp x Wp padded images, built
// once per geometry on the context's stream (stream order makes it visible to
// the GEMM that follows)
inline int get_ktab(tns_ctx* c, int64_t C, int64_t Hp, int64_t Wp, int64_t kH, int64_t kW,
                    int64_t dY, int64_t dX, const int** out) {
  auto key = std::make_tuple(C, Hp, Wp, kH, kW, dY, dX);
  auto it = c->ktabs.find(key);
  if (it != c->ktabs.end()) {
    *out = it->second;
    return TNS_OK;
  }
  const int64_t K = C * kH * kW;
  int* t = nullptr;
  hipError_t e = hipMalloc(&t, (size_t)(K + KTAB_PAD) * 2 * sizeof(int));
  if (e != hipSuccess)
    return set_error(TNS_ERR_NOMEM, "hipMalloc(k-table) failed: %s", hipGetErrorString(e));
  e = launch_build_ktab(t, (int)C, (int)Hp, (int)Wp, (int)kH, (int)kW, (int)dY, (int)dX,
                        c->stream);
  if (e != hipSuccess) {
    hipFree(t);
    return set_error(TNS_ERR_HIP, "k-table launch failed: %s", hipGetErrorString(e));
  }
  c->ktabs.emplace(key, t);
  *out = t;
  return TNS_OK;
}

}  // namespace tns
