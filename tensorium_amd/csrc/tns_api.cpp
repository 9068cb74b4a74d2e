// tns_api.cpp — the C ABI of libtensorium_hip.so (declared in include/tns.h).
//
// Host-side logic of the reference's hot path, restated for HIP:
//   * boundary A: op-table drop-ins with host pointers (cblas_sgemm & co,
//     ntensors.pas:345-385) staging through device scratch owned here;
//   * boundary B: the TNNCuda<T>-shaped device API (nncuda.pas:35-157);
//   * the options (tns_set_option), contexts and the error channel.
// The convolutional layer drivers are in conv_api.cpp; what both files share
// is in tns_ctx.hpp.  Nothing here falls back to the CPU: every compute entry point launches a
// gfx950 kernel or fails with a status.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <thread>
#include <vector>
#include <string>
#include <tuple>

#include "tns_ctx.hpp"

namespace tns {

static thread_local std::string g_err;
static tns_error_hook_t g_hook = nullptr;
static bool env_on(const char* name) { return !(getenv(name) && getenv(name)[0] == '0'); }
Options g_opt = [] {
  Options o;
  o.dx_c1 = env_on("TNS_DX_C1");
  o.bn_fused = env_on("TNS_BN_FUSED");
  return o;
}();

int set_error(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  if (g_hook) g_hook(code, buf);
  return code;
}

const char* hip_err_str(hipError_t e) { return hipGetErrorString(e); }

}  // namespace tns

using namespace tns;

namespace {
// a matrix operand of a (strided-batched) GEMM: rows x cols with leading
// dimension ld, batch copies every stride
Span span_mat(const float* p, int64_t rows, int64_t cols, int64_t ld, int64_t stride,
              int64_t batch) {
  if (rows <= 0 || cols <= 0 || batch <= 0 || !p) return Span{};
  // (a negative stride puts the later copies below p)
  const int64_t back = stride < 0 ? (batch - 1) * stride : 0;
  return span(p + back, (stride > 0 ? (batch - 1) * stride : -back) + (rows - 1) * ld + cols);
}

// ---- default context for the host-pointer API (boundary A) ---------------
std::once_flag g_default_once;
tns_ctx* g_default = nullptr;
int g_default_status = TNS_OK;

tns_ctx* default_ctx() {
  std::call_once(g_default_once, [] {
    int dev = 0;
    hipGetDevice(&dev);
    g_default_status = tns_hip_create(dev, &g_default);
  });
  return g_default_status == TNS_OK ? g_default : nullptr;
}


// ---- boundary A: the host-pointer GEMM pipeline ----------------------------
// Operands arrive in host memory.  On the MI355X box PCIe moves ~56 GB/s in
// either direction and no more with both at once (pageable and pinned alike;
// scripts/pcie_probe.py, profiles/r02_pcie.json), so the copies bound the call
// and the GEMM is hidden under them: the call is cut into chunks — rows of C
// for a single GEMM (B, which every row needs, goes first), whole GEMMs for a
// batch — and chunk j computes on the context's stream while chunk j+1
// uploads and chunk j-1 downloads on the copy stream.  Device operands keep
// the host layout (same element offsets) in context scratch; C is copied
// back row by row (2-D copies) so host gaps between rows / GEMMs are never
// overwritten.
struct HostGemm {
  bool ta, tb;
  int64_t M, N, K;
  float alpha, beta;
  const float* A;
  int64_t lda, sA;
  const float* B;
  int64_t ldb, sB;
  float* C;
  int64_t ldc, sC;
  int64_t batch;
};

int64_t span_of(int64_t rows, int64_t ld, int64_t cols) {
  return rows > 0 && cols > 0 ? (rows - 1) * ld + cols : 0;
}

// rows x cols sub-matrix with row pitch ld, same element offsets on both sides
hipError_t copy_rows(float* dst, const float* src, int64_t rows, int64_t cols, int64_t ld,
                     hipMemcpyKind kind, hipStream_t s) {
  if (rows <= 0 || cols <= 0) return hipSuccess;
  if (cols == ld || rows == 1)
    return hipMemcpyAsync(dst, src, (size_t)span_of(rows, ld, cols) * 4, kind, s);
  return hipMemcpy2DAsync(dst, (size_t)ld * 4, src, (size_t)ld * 4, (size_t)cols * 4,
                          (size_t)rows, kind, s);
}

// GEMMs [b0, b1) of a strided operand (rows x cols, pitch ld, stride st)
hipError_t copy_batch(float* dst, const float* src, int64_t b0, int64_t b1, int64_t rows,
                      int64_t cols, int64_t ld, int64_t st, hipMemcpyKind kind, hipStream_t s) {
  const int64_t one = span_of(rows, ld, cols);
  if (b1 <= b0 || one == 0) return hipSuccess;
  const bool dense = (cols == ld || rows == 1) && (st == one || b1 - b0 == 1);
  if (dense)
    return hipMemcpyAsync(dst + b0 * st, src + b0 * st, (size_t)((b1 - b0 - 1) * st + one) * 4,
                          kind, s);
  for (int64_t b = b0; b < b1; ++b)
    if (hipError_t e = copy_rows(dst + b * st, src + b * st, rows, cols, ld, kind, s)) return e;
  return hipSuccess;
}

int ensure_copy_stream(tns_ctx* c, int nev) {
  if (!c->copy_stream)
    TNS_HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  while ((int)c->pipe_ev.size() < nev) {
    hipEvent_t e;
    TNS_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->pipe_ev.push_back(e);
  }
  return TNS_OK;
}

int host_gemm_pipeline(tns_ctx* c, const HostGemm& g, int64_t R, float* dA, float* dB, float* dC,
                       const float* dA_pre, const float* dB_pre, int64_t oneA, int64_t oneB,
                       hipStream_t cs, hipStream_t ks);

// dA_pre / dB_pre: device copies of a shared (stride 0) operand already on this
// context's device (multi-device broadcast), or nullptr
int host_gemm(tns_ctx* c, const HostGemm& g, const float* dA_pre, const float* dB_pre) {
  std::lock_guard<std::mutex> lk(c->mu);
  TNS_HIP_TRY(hipSetDevice(c->device));
  const int64_t a_rows = g.ta ? g.K : g.M, a_cols = g.ta ? g.M : g.K;
  const int64_t b_rows = g.tb ? g.N : g.K, b_cols = g.tb ? g.K : g.N;
  const int64_t oneA = span_of(a_rows, g.lda, a_cols), oneB = span_of(b_rows, g.ldb, b_cols);
  const int64_t oneC = span_of(g.M, g.ldc, g.N);
  // one block of A / B serving every chunk: B of a single GEMM (chunked by
  // rows of C, which need all of B) and stride-0 operands of a batch
  const bool sharedA = g.sA == 0 || g.batch == 1, sharedB = g.sB == 0 || g.batch == 1;
  const int64_t nA = sharedA ? oneA : (g.batch - 1) * g.sA + oneA;
  const int64_t nB = sharedB ? oneB : (g.batch - 1) * g.sB + oneB;
  const int64_t nC = (g.batch - 1) * g.sC + oneC;
  float *dA = nullptr, *dB = nullptr, *dC = nullptr;
  if (!dA_pre && oneA)
    if (int r = ensure_scratch(c, SLOT_STAGE1, nA, &dA)) return r;
  if (!dB_pre && oneB)
    if (int r = ensure_scratch(c, SLOT_STAGE2, nB, &dB)) return r;
  if (int r = ensure_scratch(c, SLOT_STAGE3, nC, &dC)) return r;
  // chunks: rows of C for one GEMM (>= 512 rows each, at most 4), GEMMs for
  // a batch (at most 16)
  const bool by_rows = g.batch == 1;
  int64_t R = by_rows ? std::min<int64_t>(4, std::max<int64_t>(1, g.M / 512))
                      : std::min<int64_t>(16, g.batch);
  if (int r = ensure_copy_stream(c, (int)(2 * R))) return r;
  hipStream_t cs = c->copy_stream, ks = c->stream;
  // every path out after the first copy is enqueued drains both streams: an
  // error must not leave an upload reading (or a download writing) the
  // caller's host buffers after the call has returned
  const int r = host_gemm_pipeline(c, g, R, dA, dB, dC, dA_pre, dB_pre, oneA, oneB, cs, ks);
  if (r != TNS_OK) {
    (void)hipStreamSynchronize(cs);
    (void)hipStreamSynchronize(ks);
  }
  return r;
}

int host_gemm_pipeline(tns_ctx* c, const HostGemm& g, int64_t R, float* dA, float* dB, float* dC,
                       const float* dA_pre, const float* dB_pre, int64_t oneA, int64_t oneB,
                       hipStream_t cs, hipStream_t ks) {
  const float* uA = dA_pre ? dA_pre : dA;
  const float* uB = dB_pre ? dB_pre : dB;
  const int64_t a_rows = g.ta ? g.K : g.M, a_cols = g.ta ? g.M : g.K;
  const int64_t b_rows = g.tb ? g.N : g.K, b_cols = g.tb ? g.K : g.N;
  const bool sharedA = g.sA == 0 || g.batch == 1, sharedB = g.sB == 0 || g.batch == 1;
  const bool upfrontA = g.sA == 0 && g.batch > 1;
  const bool by_rows = g.batch == 1;
  const int64_t units = by_rows ? g.M : g.batch;
  const bool needC = beta_mode_for(g.beta) != BETA_ZERO;
  const hipMemcpyKind H2D = hipMemcpyHostToDevice, D2H = hipMemcpyDeviceToHost;
  // shared operands first
  if (!dA_pre && upfrontA && oneA)
    TNS_HIP_TRY(copy_rows(dA, g.A, a_rows, a_cols, g.lda, H2D, cs));
  if (!dB_pre && sharedB && oneB)
    TNS_HIP_TRY(copy_rows(dB, g.B, b_rows, b_cols, g.ldb, H2D, cs));
  auto lo = [&](int64_t j) { return units * j / R; };
  auto download = [&](int64_t j) -> hipError_t {
    const int64_t u0 = lo(j), u1 = lo(j + 1);
    if (by_rows)
      return copy_rows(g.C + u0 * g.ldc, dC + u0 * g.ldc, u1 - u0, g.N, g.ldc, D2H, cs);
    return copy_batch(g.C, dC, u0, u1, g.M, g.N, g.ldc, g.sC, D2H, cs);
  };
  for (int64_t j = 0; j < R; ++j) {
    const int64_t u0 = lo(j), u1 = lo(j + 1);
    hipEvent_t up = c->pipe_ev[2 * j], done = c->pipe_ev[2 * j + 1];
    if (by_rows) {  // rows u0..u1 of C: rows of A (NoTrans) or its columns (Trans)
      if (!dA_pre && oneA) {
        if (g.ta)
          TNS_HIP_TRY(copy_rows(dA + u0, g.A + u0, g.K, u1 - u0, g.lda, H2D, cs));
        else
          TNS_HIP_TRY(copy_rows(dA + u0 * g.lda, g.A + u0 * g.lda, u1 - u0, g.K, g.lda, H2D, cs));
      }
      if (needC)
        TNS_HIP_TRY(copy_rows(dC + u0 * g.ldc, g.C + u0 * g.ldc, u1 - u0, g.N, g.ldc, H2D, cs));
    } else {
      if (!sharedA) TNS_HIP_TRY(copy_batch(dA, g.A, u0, u1, a_rows, a_cols, g.lda, g.sA, H2D, cs));
      if (!sharedB) TNS_HIP_TRY(copy_batch(dB, g.B, u0, u1, b_rows, b_cols, g.ldb, g.sB, H2D, cs));
      if (needC) TNS_HIP_TRY(copy_batch(dC, g.C, u0, u1, g.M, g.N, g.ldc, g.sC, H2D, cs));
    }
    TNS_HIP_TRY(hipEventRecord(up, cs));
    TNS_HIP_TRY(hipStreamWaitEvent(ks, up, 0));
    int r;
    if (by_rows)
      r = do_gemm(c, g.ta, g.tb, u1 - u0, g.N, g.K, g.alpha,
                  uA ? uA + (g.ta ? u0 : u0 * g.lda) : nullptr, g.lda, 0, uB, g.ldb, 0, g.beta,
                  dC + u0 * g.ldc, g.ldc, 0, 1, EPI_NONE, nullptr, 0);
    else
      r = do_gemm(c, g.ta, g.tb, g.M, g.N, g.K, g.alpha, uA ? uA + (sharedA ? 0 : u0 * g.sA) : nullptr,
                  g.lda, sharedA ? 0 : g.sA, uB ? uB + (sharedB ? 0 : u0 * g.sB) : nullptr, g.ldb,
                  sharedB ? 0 : g.sB, g.beta, dC + u0 * g.sC, g.ldc, g.sC, u1 - u0, EPI_NONE,
                  nullptr, 0);
    if (r) return r;
    TNS_HIP_TRY(hipEventRecord(done, ks));
    if (j > 0) {
      TNS_HIP_TRY(hipStreamWaitEvent(cs, c->pipe_ev[2 * j - 1], 0));
      TNS_HIP_TRY(download(j - 1));
    }
  }
  TNS_HIP_TRY(hipStreamWaitEvent(cs, c->pipe_ev[2 * R - 1], 0));
  TNS_HIP_TRY(download(R - 1));
  TNS_HIP_TRY(hipStreamSynchronize(cs));
  return TNS_OK;
}

// ---- several GPUs from one process (sgemm_strided_batched_multi)
// Slot i of a call owns a context on devices[i] (two slots may share a
// device); the batch is split into contiguous shards, the first batch % n
// slots one GEMM longer (tensorium_amd/shard.py, the reference's MP.&For
// blocks).  A shared operand (stride 0: the conv weights of
// nConvolutionLayer.pas:773) crosses PCIe once, to slot 0, and reaches the
// other devices by peer copies over xGMI.  Each slot runs the host pipeline
// above on its own host thread.
std::mutex g_pool_mu;
std::vector<tns_ctx*> g_pool;
std::mutex g_op_devices_mu;
std::vector<int32_t> g_op_devices;

int pool_ctx(int slot, int device, tns_ctx** out) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  if ((int)g_pool.size() <= slot) g_pool.resize(slot + 1, nullptr);
  if (g_pool[slot] && g_pool[slot]->device != device) {
    tns_hip_destroy(g_pool[slot]);
    g_pool[slot] = nullptr;
  }
  if (!g_pool[slot])
    if (int r = tns_hip_create(device, &g_pool[slot])) return r;
  *out = g_pool[slot];
  return TNS_OK;
}

int multi_host_gemm(const int32_t* devices, int n, const HostGemm& g) {
  std::vector<tns_ctx*> ctx(n);
  for (int i = 0; i < n; ++i)
    if (int r = pool_ctx(i, devices[i], &ctx[i])) return r;
  const int64_t a_rows = g.ta ? g.K : g.M, a_cols = g.ta ? g.M : g.K;
  const int64_t b_rows = g.tb ? g.N : g.K, b_cols = g.tb ? g.K : g.N;
  const int64_t oneA = span_of(a_rows, g.lda, a_cols), oneB = span_of(b_rows, g.ldb, b_cols);
  // shared operands: host -> slot 0 once, slot 0 -> every other slot by peer
  // copy; only the slots that get GEMMs (the first min(n, batch)) need them,
  // and with one such slot (a single GEMM: the op-table's plain gemm) there is
  // nothing to broadcast: slot 0 runs the ordinary pipeline, row-chunked
  // uploads included
  const int nwork = (int)std::min<int64_t>(n, g.batch);
  std::vector<const float*> preA(n, nullptr), preB(n, nullptr);
  auto broadcast = [&](const float* host, int64_t rows, int64_t cols, int64_t ld, int64_t elems,
                       int slot, std::vector<const float*>& pre) -> int {
    float* root;
    {
      std::lock_guard<std::mutex> lk(ctx[0]->mu);
      TNS_HIP_TRY(hipSetDevice(ctx[0]->device));
      if (int r = ensure_scratch(ctx[0], slot, elems, &root)) return r;
      TNS_HIP_TRY(copy_rows(root, host, rows, cols, ld, hipMemcpyHostToDevice, ctx[0]->stream));
      TNS_HIP_TRY(hipStreamSynchronize(ctx[0]->stream));
    }
    pre[0] = root;
    for (int i = 1; i < nwork; ++i) {
      std::lock_guard<std::mutex> lk(ctx[i]->mu);
      TNS_HIP_TRY(hipSetDevice(ctx[i]->device));
      float* d;
      if (int r = ensure_scratch(ctx[i], slot, elems, &d)) return r;
      if (ctx[i]->device == ctx[0]->device)
        TNS_HIP_TRY(hipMemcpyAsync(d, root, (size_t)elems * 4, hipMemcpyDeviceToDevice,
                                   ctx[i]->stream));
      else
        TNS_HIP_TRY(hipMemcpyPeerAsync(d, ctx[i]->device, root, ctx[0]->device,
                                       (size_t)elems * 4, ctx[i]->stream));
      TNS_HIP_TRY(hipStreamSynchronize(ctx[i]->stream));
      pre[i] = d;
    }
    return TNS_OK;
  };
  if (g.sA == 0 && oneA && nwork > 1)
    if (int r = broadcast(g.A, a_rows, a_cols, g.lda, oneA, SLOT_STAGE1, preA)) return r;
  if (g.sB == 0 && oneB && nwork > 1)
    if (int r = broadcast(g.B, b_rows, b_cols, g.ldb, oneB, SLOT_STAGE2, preB)) return r;
  std::vector<int> status(n, TNS_OK);
  std::vector<std::string> errs(n);
  std::vector<std::thread> th;
  const int64_t base = g.batch / n, extra = g.batch % n;
  for (int i = 0; i < n; ++i) {
    const int64_t s0 = i * base + std::min<int64_t>(i, extra);
    const int64_t cnt = base + (i < extra ? 1 : 0);
    if (cnt == 0) continue;
    HostGemm gi = g;
    gi.A = g.sA ? g.A + s0 * g.sA : g.A;
    gi.B = g.sB ? g.B + s0 * g.sB : g.B;
    gi.C = g.C + s0 * g.sC;
    gi.batch = cnt;
    th.emplace_back([&, i, gi] {
      status[i] = host_gemm(ctx[i], gi, preA[i], preB[i]);
      if (status[i]) errs[i] = g_err;  // the error string is thread-local
    });
  }
  for (auto& t : th) t.join();
  for (int i = 0; i < n; ++i)
    if (status[i]) return set_error(status[i], "slot %d (device %d): %s", i, devices[i],
                                    errs[i].c_str());
  return TNS_OK;
}

}  // namespace

extern "C" {

int tns_abi_version(void) { return TNS_ABI_VERSION; }
const char* tns_last_error(void) { return g_err.c_str(); }
void tns_clear_error(void) { g_err.clear(); }
void tns_set_error_hook(tns_error_hook_t hook) { g_hook = hook; }

int tns_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int tns_set_option(int32_t opt, int64_t value) {
  switch (opt) {
    case TNS_OPT_STRICT_BETA0:
      g_opt.strict_beta0 = value ? 1 : 0;
      return TNS_OK;
    case TNS_OPT_CONV_VARIANT:
      g_opt.conv_variant = value < 0 ? -1 : value;
      return TNS_OK;
    case TNS_OPT_CONV_PAD:
      g_opt.conv_pad = value < 0 ? -1 : (value ? 1 : 0);
      return TNS_OK;
    case TNS_OPT_NT_SDOT:
      g_opt.nt_sdot = value ? 1 : 0;
      return TNS_OK;
    case TNS_OPT_SRSS_QUIRK:
      g_opt.srss_quirk = value ? 1 : 0;
      return TNS_OK;
    case TNS_OPT_TT_EXACT:
      g_opt.tt_exact = value ? 1 : 0;
      return TNS_OK;
    case TNS_OPT_SDOT_FORM:
      if (value > sdot_chains_variant_count() &&
          (value < SDOT_FORM_RC || value >= SDOT_FORM_RC + sdot_rc_variant_count()))
        return set_error(TNS_ERR_ARG, "sdot form %lld out of range", (long long)value);
      set_sdot_form((int)value);
      return TNS_OK;
    case TNS_OPT_DX_FUSED:
      g_opt.dx_fused = value < 0 ? 1 : (value > 2 ? 2 : value);
      return TNS_OK;
    case TNS_OPT_BWD_OVERLAP:
      g_opt.bwd_overlap = value <= 0 ? 0 : (value >= 2 ? 2 : 1);
      return TNS_OK;
    case TNS_OPT_DW_TILE:
      if (value >= dw_tile_count()) return set_error(TNS_ERR_ARG, "no dW tile %lld", (long long)value);
      g_opt.dw_tile = value < -1 ? -2 : value;
      return TNS_OK;
    case TNS_OPT_DX_TILE:
      if (value >= conv_tile4_ta_count()) return set_error(TNS_ERR_ARG, "no dX tile %lld", (long long)value);
      g_opt.dx_tile = value < -1 ? -2 : value;
      return TNS_OK;
    case TNS_OPT_DW_RES:
      if (value >= dw_res_count()) return set_error(TNS_ERR_ARG, "no dW res form %lld", (long long)value);
      g_opt.dw_res = value < -1 ? -2 : value;
      return TNS_OK;
    case TNS_OPT_DERIVE_SUMS:
      g_opt.derive_sums = value ? 1 : 0;
      return TNS_OK;
    case TNS_OPT_SCRATCH_CAP:
      g_opt.scratch_cap = value > 0 ? value : 0;
      return TNS_OK;
    case TNS_OPT_DX_CONV:
      if (value >= conv_tile4_dx3_count())
        return set_error(TNS_ERR_ARG, "no dX conv form %lld", (long long)value);
      g_opt.dx_conv = value < -1 ? -2 : value;
      return TNS_OK;
    default:
      return set_error(TNS_ERR_ARG, "unknown option %d", opt);
  }
}

// ---- context ---------------------------------------------------------------
int tns_hip_create(int32_t deviceIndex, tns_ctx** out) {
  if (!out) return set_error(TNS_ERR_ARG, "tns_hip_create: null out");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return set_error(TNS_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (deviceIndex < 0 || deviceIndex >= n)
    return set_error(TNS_ERR_ARG, "device index %d out of range [0,%d)", deviceIndex, n);
  TNS_HIP_TRY(hipSetDevice(deviceIndex));
  tns_ctx* c = new tns_ctx();
  c->device = deviceIndex;
  {
    int least = 0, greatest = 0;
    const char* sp = getenv("TNS_STREAM_PRIO");  // (see ensure_side_stream)
    if (!(sp && sp[0] == '0') &&
        hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess)
      e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, greatest);
    else
      e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  }
  if (e != hipSuccess) {
    delete c;
    return set_error(TNS_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
  }
  c->own_stream = true;
  hipEventCreate(&c->ev0);
  hipEventCreate(&c->ev1);
  *out = c;
  return TNS_OK;
}

int tns_hip_destroy(tns_ctx* c) {
  if (!c) return TNS_OK;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->aux_stream) hipStreamSynchronize(c->aux_stream);
  if (c->ovl_stream) hipStreamSynchronize(c->ovl_stream);
  for (int i = 0; i < tns_ctx::kSlots; ++i)
    if (c->scratch[i]) hipFree(c->scratch[i]);
  for (auto& kv : c->ktabs) hipFree(kv.second);
  if (c->ev0) hipEventDestroy(c->ev0);
  if (c->ev1) hipEventDestroy(c->ev1);
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
  if (c->copy_stream) hipStreamDestroy(c->copy_stream);
  if (c->aux_stream) hipStreamDestroy(c->aux_stream);
  if (c->ovl_stream) hipStreamDestroy(c->ovl_stream);
  if (c->ev_fork) hipEventDestroy(c->ev_fork);
  if (c->ev_join) hipEventDestroy(c->ev_join);
  for (hipEvent_t e : c->pipe_ev) hipEventDestroy(e);
  delete c;
  return TNS_OK;
}

int tns_hip_set_stream(tns_ctx* c, void* s) {
  if (int r = check_ctx(c)) return r;
  if (c->own_stream && c->stream) {
    hipStreamSynchronize(c->stream);
    hipStreamDestroy(c->stream);
  }
  c->stream = (hipStream_t)s;
  c->own_stream = false;
  return TNS_OK;
}

void* tns_hip_get_stream(tns_ctx* c) {
  // (pipelined backward: work the caller enqueues on the stream must see
  // the pending dW products' weight_updates — join them first)
  if (!c || join_side(c)) return nullptr;
  return (void*)c->stream;
}

int tns_hip_pending_dw(tns_ctx* c) {
  if (!c) return -1;
  return c->side_pending ? (int)c->pending.size() : 0;
}

int tns_hip_finish(tns_ctx* c) {
  if (int r = check_ctx(c)) return r;
  return hip_status(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
}

int tns_hip_malloc(tns_ctx* c, int64_t n, float** out) {
  if (int r = check_ctx(c)) return r;
  if (!out || n < 0) return set_error(TNS_ERR_ARG, "tns_hip_malloc: bad args");
  hipError_t e = hipMalloc((void**)out, (size_t)(n > 0 ? n : 1) * sizeof(float));
  if (e != hipSuccess) return set_error(TNS_ERR_NOMEM, "hipMalloc: %s", hipGetErrorString(e));
  return TNS_OK;
}

int tns_hip_free(tns_ctx* c, float* p) {
  if (int r = check_ctx(c)) return r;
  return hip_status(hipFree(p), "hipFree");
}

int tns_hip_write_buffer(tns_ctx* c, float* dev, int64_t bytes, const void* host) {
  if (int r = check_ctx(c)) return r;
  if (bytes <= 0) return TNS_OK;
  TNS_HIP_TRY(hipMemcpyAsync(dev, host, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
  return hip_status(hipStreamSynchronize(c->stream), "writeBuffer sync");
}

int tns_hip_read_buffer(tns_ctx* c, const float* dev, int64_t bytes, void* host) {
  if (int r = check_ctx(c)) return r;
  if (bytes <= 0) return TNS_OK;
  TNS_HIP_TRY(hipMemcpyAsync(host, dev, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
  return hip_status(hipStreamSynchronize(c->stream), "readBuffer sync");
}

// ---- boundary B: device API ---------------------------------------------------
int tns_hip_gemm(tns_ctx* c, uint8_t transA, uint8_t transB, int64_t M, int64_t N, int64_t K,
                 float ALPHA, const float* A, int64_t aOffset, int64_t lda, const float* B,
                 int64_t bOffset, int64_t ldb, float BETA, float* C, int64_t cOffset,
                 int64_t ldc) {
  if (int r = check_ops(c, {span_mat(C ? C + cOffset : nullptr, M, N, ldc, 0, 1)},
                        {transA ? span_mat(A ? A + aOffset : nullptr, K, M, lda, 0, 1)
                                : span_mat(A ? A + aOffset : nullptr, M, K, lda, 0, 1),
                         transB ? span_mat(B ? B + bOffset : nullptr, N, K, ldb, 0, 1)
                                : span_mat(B ? B + bOffset : nullptr, K, N, ldb, 0, 1)}))
    return r;
  return do_gemm(c, transA != 0, transB != 0, M, N, K, ALPHA, A ? A + aOffset : nullptr, lda, 0,
                 B ? B + bOffset : nullptr, ldb, 0, BETA, C ? C + cOffset : nullptr, ldc, 0, 1,
                 EPI_NONE, nullptr, 0);
}

int tns_hip_gemm_strided_batched(tns_ctx* c, uint8_t transA, uint8_t transB, int64_t M,
                                 int64_t N, int64_t K, float ALPHA, const float* A,
                                 int64_t aOffset, int64_t lda, int64_t strideA, const float* B,
                                 int64_t bOffset, int64_t ldb, int64_t strideB, float BETA,
                                 float* C, int64_t cOffset, int64_t ldc, int64_t strideC,
                                 int64_t batchCount) {
  if (int r = check_ops(
          c, {span_mat(C ? C + cOffset : nullptr, M, N, ldc, strideC, batchCount)},
          {transA ? span_mat(A ? A + aOffset : nullptr, K, M, lda, strideA, batchCount)
                  : span_mat(A ? A + aOffset : nullptr, M, K, lda, strideA, batchCount),
           transB ? span_mat(B ? B + bOffset : nullptr, N, K, ldb, strideB, batchCount)
                  : span_mat(B ? B + bOffset : nullptr, K, N, ldb, strideB, batchCount)}))
    return r;
  return do_gemm(c, transA != 0, transB != 0, M, N, K, ALPHA, A ? A + aOffset : nullptr, lda,
                 strideA, B ? B + bOffset : nullptr, ldb, strideB, BETA,
                 C ? C + cOffset : nullptr, ldc, strideC, batchCount, EPI_NONE, nullptr, 0);
}

int tns_hip_gemm_batched(tns_ctx* c, uint8_t transA, uint8_t transB, int64_t M, int64_t N,
                         int64_t K, float ALPHA, const float* const* A, int64_t aOffset,
                         int64_t lda, const float* const* B, int64_t bOffset, int64_t ldb,
                         float BETA, float* const* C, int64_t cOffset, int64_t ldc,
                         int64_t batchCount) {
  if (int r = check_ctx(c)) return r;
  if (batchCount < 0) return set_error(TNS_ERR_ARG, "gemmBatched: batchCount < 0");
  if (batchCount == 0) return TNS_OK;
  if (!A || !B || !C) return set_error(TNS_ERR_ARG, "gemmBatched: null pointer array");
  // The pointer arrays are read where they live (hipMemcpyDefault: device
  // arrays written by writeBuffer as nConvolutionLayer.pas:1083-1085 builds
  // them, or host arrays), in stream order after the work that wrote them.
  const size_t bytes = (size_t)batchCount * sizeof(void*);
  std::vector<const float*> pa(batchCount), pb(batchCount);
  std::vector<float*> pc(batchCount);
  TNS_HIP_TRY(hipSetDevice(c->device));
  TNS_HIP_TRY(hipMemcpyAsync(pa.data(), A, bytes, hipMemcpyDefault, c->stream));
  TNS_HIP_TRY(hipMemcpyAsync(pb.data(), B, bytes, hipMemcpyDefault, c->stream));
  TNS_HIP_TRY(hipMemcpyAsync(pc.data(), C, bytes, hipMemcpyDefault, c->stream));
  TNS_HIP_TRY(hipStreamSynchronize(c->stream));
  for (int64_t i = 0; i < batchCount; ++i)
    if (!pa[i] || !pb[i] || !pc[i])
      return set_error(TNS_ERR_ARG, "gemmBatched: null matrix pointer at entry %lld", (long long)i);
  // equally spaced entries (the common case: slices of one buffer) run as one
  // strided-batched launch; anything else GEMM by GEMM in array order
  auto stride_of = [&](auto& v, int64_t* st) {
    const intptr_t d = batchCount > 1 ? (const char*)v[1] - (const char*)v[0] : 0;
    if (d < 0 || d % (intptr_t)sizeof(float)) return false;
    for (int64_t i = 2; i < batchCount; ++i)
      if ((const char*)v[i] - (const char*)v[i - 1] != d) return false;
    *st = (int64_t)(d / (intptr_t)sizeof(float));
    return true;
  };
  // — only when the batch's GEMMs are independent: the C entries do not
  // overlap one another and no C entry overlaps an A or B entry (the launch
  // runs them concurrently; the loop below keeps the array order)
  const int64_t extA = transA ? (K - 1) * lda + M : (M - 1) * lda + K;
  const int64_t extB = transB ? (N - 1) * ldb + K : (K - 1) * ldb + N;
  const int64_t extC = (M - 1) * ldc + N;
  auto disjoint = [](const float* p, int64_t n, const float* q, int64_t m) {
    return p + n <= q || q + m <= p;
  };
  int64_t sA, sB, sC;
  if (stride_of(pa, &sA) && stride_of(pb, &sB) && stride_of(pc, &sC) &&
      (batchCount == 1 || sC >= extC) &&
      disjoint(pc[0] + cOffset, sC * (batchCount - 1) + extC, pa[0] + aOffset,
               sA * (batchCount - 1) + extA) &&
      disjoint(pc[0] + cOffset, sC * (batchCount - 1) + extC, pb[0] + bOffset,
               sB * (batchCount - 1) + extB))
    return do_gemm(c, transA != 0, transB != 0, M, N, K, ALPHA, pa[0] + aOffset, lda, sA,
                   pb[0] + bOffset, ldb, sB, BETA, pc[0] + cOffset, ldc, sC, batchCount, EPI_NONE,
                   nullptr, 0);
  for (int64_t i = 0; i < batchCount; ++i)
    if (int r = do_gemm(c, transA != 0, transB != 0, M, N, K, ALPHA, pa[i] + aOffset, lda, 0,
                        pb[i] + bOffset, ldb, 0, BETA, pc[i] + cOffset, ldc, 0, 1, EPI_NONE,
                        nullptr, 0))
      return r;
  return TNS_OK;
}

int tns_hip_im2col_strided_batched(tns_ctx* c, int64_t aChannels, int64_t aHeight,
                                   int64_t aWidth, int64_t kernelHeight, int64_t kernelWidth,
                                   int64_t padHeight, int64_t padWidth, int64_t strideY,
                                   int64_t strideX, int64_t dilationY, int64_t dilationX,
                                   const float* im, int64_t imStride, int64_t imOffset,
                                   float* col, int64_t colStride, int64_t colOffset,
                                   int64_t batchCount) {
  if (!c) return check_ctx(c);
  ConvGeom g = geom(aChannels, aHeight, aWidth, kernelHeight, kernelWidth, padHeight, padWidth,
                    strideY, strideX, dilationY, dilationX);
  if (int r = check_geom(g)) return r;
  if (!im || !col) return set_error(TNS_ERR_ARG, "im2col: null pointer");
  {
    const int64_t nb = batchCount > 0 ? batchCount : 0, colN = g.C * g.kH * g.kW * g.oh * g.ow;
    if (int r = check_ops(c, {span_mat(col + colOffset, 1, colN, colN, colStride, nb)},
                          {span_mat(im + imOffset, 1, g.C * g.H * g.W, 0, imStride, nb)}))
      return r;
  }
  OpTimer t(c, TNS_OP_IM2COL);
  return hip_status(launch_im2col(g, im + imOffset, imStride, col + colOffset, colStride,
                                  batchCount, c->stream),
                    "im2col launch");
}

int tns_hip_im2col(tns_ctx* c, int64_t aChannels, int64_t aHeight, int64_t aWidth,
                   int64_t kernelHeight, int64_t kernelWidth, int64_t padHeight, int64_t padWidth,
                   int64_t strideY, int64_t strideX, int64_t dilationY, int64_t dilationX,
                   const float* im, int64_t imOffset, float* col, int64_t colOffset) {
  return tns_hip_im2col_strided_batched(c, aChannels, aHeight, aWidth, kernelHeight, kernelWidth,
                                        padHeight, padWidth, strideY, strideX, dilationY,
                                        dilationX, im, 0, imOffset, col, 0, colOffset, 1);
}

int tns_hip_col2im_strided_batched(tns_ctx* c, int64_t aChannels, int64_t aHeight,
                                   int64_t aWidth, int64_t kernelHeight, int64_t kernelWidth,
                                   int64_t padHeight, int64_t padWidth, int64_t strideY,
                                   int64_t strideX, int64_t dilationY, int64_t dilationX,
                                   const float* col, int64_t colStride, int64_t colOffset,
                                   float* im, int64_t imStride, int64_t imOffset,
                                   int64_t batchCount) {
  if (!c) return check_ctx(c);
  ConvGeom g = geom(aChannels, aHeight, aWidth, kernelHeight, kernelWidth, padHeight, padWidth,
                    strideY, strideX, dilationY, dilationX);
  if (int r = check_geom(g)) return r;
  if (!im || !col) return set_error(TNS_ERR_ARG, "col2im: null pointer");
  {
    const int64_t nb = batchCount > 0 ? batchCount : 0, colN = g.C * g.kH * g.kW * g.oh * g.ow;
    if (int r = check_ops(c, {span_mat(im + imOffset, 1, g.C * g.H * g.W, 0, imStride, nb)},
                          {span_mat(col + colOffset, 1, colN, colN, colStride, nb)}))
      return r;
  }
  if (batchCount > 1 && imStride < aChannels * aHeight * aWidth)
    return set_error(TNS_ERR_ARG, "col2im: overlapping image strides");
  OpTimer t(c, TNS_OP_COL2IM);
  return hip_status(launch_col2im(g, col + colOffset, colStride, im + imOffset, imStride,
                                  batchCount, c->stream),
                    "col2im launch");
}

int tns_hip_col2im(tns_ctx* c, int64_t aChannels, int64_t aHeight, int64_t aWidth,
                   int64_t kernelHeight, int64_t kernelWidth, int64_t padHeight, int64_t padWidth,
                   int64_t strideY, int64_t strideX, int64_t dilationY, int64_t dilationX,
                   const float* col, int64_t colOffset, float* im, int64_t imOffset) {
  return tns_hip_col2im_strided_batched(c, aChannels, aHeight, aWidth, kernelHeight, kernelWidth,
                                        padHeight, padWidth, strideY, strideX, dilationY,
                                        dilationX, col, 0, colOffset, im, 0, imOffset, 1);
}

int tns_hip_forward_bias(tns_ctx* c, int64_t dstSize, float* dst, int64_t offset, int64_t srcSize,
                         const float* src, int64_t incb, int64_t batch) {
  if (int r = check_ops(c, {span(dst ? dst + offset : nullptr, dstSize)}, {span(src, srcSize, incb)}))
    return r;
  if (incb < 1) return set_error(TNS_ERR_ARG, "forwardBias: incb < 1");
  if (dstSize == 0) return TNS_OK;
  if (!dst || !src || srcSize <= 0 || batch <= 0 || dstSize % (srcSize * batch) != 0)
    return set_error(TNS_ERR_ARG, "forwardBias: sizes do not align");
  const int64_t bs = dstSize / (srcSize * batch);
  OpTimer t(c, TNS_OP_BIAS);
  return hip_status(launch_forward_bias(dst + offset, srcSize, bs, src, incb, batch, c->stream),
                    "forwardBias launch");
}

int tns_hip_backward_bias(tns_ctx* c, int64_t dstSize, float* dst, int64_t srcSize,
                          const float* src, int64_t srcOffset, int64_t incb, int64_t batch) {
  if (int r = check_ops(c, {span(dst, dstSize, incb)},
                        {span(src ? src + srcOffset : nullptr, srcSize)}))
    return r;
  if (incb < 1) return set_error(TNS_ERR_ARG, "backwardBias: incb < 1");
  if (!dst || !src || dstSize <= 0 || batch <= 0 || srcSize % (dstSize * batch) != 0)
    return set_error(TNS_ERR_ARG, "backwardBias: sizes do not align");
  const int64_t bs = srcSize / (dstSize * batch);
  OpTimer t(c, TNS_OP_BIAS);
  // FC layers: the reference's sequential strided sum (one output: its
  // stride-1 sumv, whatever incb says about outputs that do not exist)
  if (bs == 1 && (incb == 1 || dstSize == 1))
    return hip_status(launch_add_sums(dst, src + srcOffset, batch, dstSize, 1, nullptr, c->stream),
                      "backwardBias launch");
  if (incb == 1 && bs >= 64) {  // conv blocks: lane chains per block
    float* part;
    if (int r = ensure_scratch(c, SLOT_BN, batch * dstSize, &part)) return r;
    return hip_status(launch_add_sums(dst, src + srcOffset, batch, dstSize, bs, part, c->stream),
                      "backwardBias launch");
  }
  return hip_status(launch_backward_bias(dst, dstSize, src + srcOffset, bs, batch, incb, c->stream),
                    "backwardBias launch");
}

int tns_hip_activate_array(tns_ctx* c, int64_t N, float* x, int64_t offset, int32_t activation) {
  if (int r = check_ops(c, {span(x ? x + offset : nullptr, N)}, {})) return r;
  if (!act_supported(activation))
    return set_error(TNS_ERR_UNSUPPORTED, "activation %d not implemented", activation);
  if (N <= 0) return TNS_OK;
  if (!x) return set_error(TNS_ERR_ARG, "activate: null pointer");
  OpTimer t(c, TNS_OP_ACTIVATE);
  return hip_status(launch_activate(x + offset, N, activation, c->stream), "activate launch");
}

int tns_hip_derive_array(tns_ctx* c, int64_t N, const float* x, int64_t offset,
                         int32_t activation, float* delta) {
  if (int r = check_ops(c, {span(delta, N)}, {span(x ? x + offset : nullptr, N)})) return r;
  if (!act_supported(activation))
    return set_error(TNS_ERR_UNSUPPORTED, "derivative %d not implemented", activation);
  if (N <= 0) return TNS_OK;
  if (!x || !delta) return set_error(TNS_ERR_ARG, "derive: null pointer");
  OpTimer t(c, TNS_OP_ACTIVATE);
  return hip_status(launch_derive(x + offset, N, activation, delta, c->stream), "derive launch");
}

int tns_hip_axpy(tns_ctx* c, int64_t N, float a, const float* x, int64_t xOffset, int64_t incx,
                 float* y, int64_t yOffset, int64_t incy) {
  if (int r = check_ops(c, {span(y ? y + yOffset : nullptr, N, incy)},
                        {span(x ? x + xOffset : nullptr, N, incx)}))
    return r;
  if (N < 0 || incx < 0 || incy < 1 || (N > 0 && (!x || !y)))
    return set_error(TNS_ERR_ARG, "axpy: bad args");
  return hip_status(launch_axpy(N, a, x + xOffset, incx, y + yOffset, incy, c->stream), "axpy");
}

int tns_hip_sgd_update(tns_ctx* c, int64_t nWeights, float* weights, float* weight_updates,
                       int64_t n, float* biases, float* bias_updates, float* scales,
                       float* scale_updates, float lrOverBatch, float negDecayTimesBatch,
                       float momentum) {
  if (int r = check_ops(c, {span(weights, nWeights), span(weight_updates, nWeights), span(biases, n),
                            span(bias_updates, n), span(scales, n), span(scale_updates, n)},
                        {}))
    return r;
  if (nWeights < 0 || n < 0 || (nWeights > 0 && (!weights || !weight_updates)) ||
      (n > 0 && (!biases || !bias_updates)) || (!scales != !scale_updates))
    return set_error(TNS_ERR_ARG, "sgd_update: bad arguments");
  return hip_status(launch_sgd_update(nWeights, weights, weight_updates, n, biases, bias_updates,
                                      n > 0 ? scales : nullptr, scale_updates, lrOverBatch,
                                      negDecayTimesBatch, momentum, c->stream),
                    "sgd_update");
}

int tns_hip_scale(tns_ctx* c, int64_t N, float a, float* x, int64_t stride) {
  if (int r = check_ops(c, {span(x, N, stride)}, {})) return r;
  if (N < 0 || stride < 1 || (N > 0 && !x)) return set_error(TNS_ERR_ARG, "scale: bad args");
  return hip_status(launch_scale(N, a, x, stride, c->stream), "scale");
}

int tns_hip_fill(tns_ctx* c, int64_t N, float* x, int64_t offset, float val, int64_t stride) {
  if (int r = check_ops(c, {span(x ? x + offset : nullptr, N, stride)}, {})) return r;
  if (N < 0 || stride < 1 || (N > 0 && !x)) return set_error(TNS_ERR_ARG, "fill: bad args");
  return hip_status(launch_fill(N, x + offset, val, stride, c->stream), "fill");
}

int tns_hip_copy(tns_ctx* c, int64_t N, const float* src, int64_t srcOffset, int64_t inca,
                 float* dst, int64_t dstOffset, int64_t incb) {
  if (int r = check_ops(c, {span(dst ? dst + dstOffset : nullptr, N, incb)},
                        {span(src ? src + srcOffset : nullptr, N, inca)}))
    return r;
  if (N < 0 || inca < 0 || incb < 1 || (N > 0 && (!src || !dst)))
    return set_error(TNS_ERR_ARG, "copy: bad args");
  return hip_status(launch_copy(N, src + srcOffset, inca, dst + dstOffset, incb, c->stream),
                    "copy");
}

int tns_hip_shortcut(tns_ctx* c, int64_t N, const float* a, int64_t aOffset, const float* b,
                     int64_t bOffset, float* out, int64_t outOffset, int32_t activation) {
  if (int r = check_ops(c, {span(out ? out + outOffset : nullptr, N)},
                        {span(a ? a + aOffset : nullptr, N), span(b ? b + bOffset : nullptr, N)}))
    return r;
  if (N < 0 || (N > 0 && (!a || !b || !out))) return set_error(TNS_ERR_ARG, "shortcut: bad args");
  if (!act_supported(activation))
    return set_error(TNS_ERR_UNSUPPORTED, "activation %d not implemented", activation);
  return hip_status(launch_shortcut(N, a + aOffset, b + bOffset, out + outOffset, activation,
                                    c->stream),
                    "shortcut");
}

int tns_hip_upsample(tns_ctx* c, int64_t aBatch, int64_t aChannels, int64_t outHeight,
                     int64_t outWidth, float* in, int64_t stride, int32_t isForward, float scale,
                     float* out, int32_t zeroIn) {
  {
    const int64_t small = aBatch * aChannels * outHeight * outWidth, big = small * stride * stride;
    const Span si = span(in, small), so = span(out, big);
    if (int r = isForward ? check_ops(c, {so}, {si}) : check_ops(c, {si}, {so})) return r;
  }
  const int64_t planes = aBatch * aChannels, H = outHeight, W = outWidth;
  if (aBatch < 0 || aChannels < 0 || H < 0 || W < 0 || stride < 1 ||
      H * stride > 0x7fffffff || W * stride > 0x7fffffff ||
      (planes * H * W > 0 && (!in || !out)))
    return set_error(TNS_ERR_ARG, "upsample: bad args");
  if (isForward)
    return hip_status(launch_upsample(planes, (int)H, (int)W, (int)stride, scale, in, out,
                                      c->stream),
                      "upsample");
  return hip_status(launch_upsample_backward(planes, (int)H, (int)W, (int)stride, scale, in, out,
                                             zeroIn, c->stream),
                    "upsample backward");
}

// TNNCuda.addvv / subvv / mulvv / fmavv / fmavss / inverseSqrt (nncuda.pas:120-151)
namespace {
int vv(tns_ctx* c, int op, int64_t N, const float* a, int64_t aOff, int64_t inca, const float* b,
       int64_t bOff, int64_t incb, const float* cc, int64_t cOff, int64_t incc, float* d,
       int64_t dOff, int64_t incd, const char* what) {
  if (int r = check_ops(c, {span(d ? d + dOff : nullptr, N, incd)},
                        {span(a ? a + aOff : nullptr, N, inca), span(b ? b + bOff : nullptr, N, incb),
                         span(cc ? cc + cOff : nullptr, N, incc)}))
    return r;
  if (N < 0 || (N > 0 && (!a || !b || !d || (op == 3 && !cc))))
    return set_error(TNS_ERR_ARG, "%s: bad args", what);
  return hip_status(launch_vv(op, N, a + aOff, inca, b + bOff, incb, cc ? cc + cOff : nullptr,
                              incc, d + dOff, incd, c->stream),
                    what);
}
}  // namespace

int tns_hip_addvv(tns_ctx* c, int64_t N, const float* src1, int64_t src1Offset, int64_t inca,
                  const float* src2, int64_t src2Offset, int64_t incb, float* dst,
                  int64_t dstOffset, int64_t incc) {
  return vv(c, 0, N, src1, src1Offset, inca, src2, src2Offset, incb, nullptr, 0, 0, dst,
            dstOffset, incc, "addvv");
}

int tns_hip_subvv(tns_ctx* c, int64_t N, const float* src1, int64_t src1Offset, int64_t inca,
                  const float* src2, int64_t src2Offset, int64_t incb, float* dst,
                  int64_t dstOffset, int64_t incc) {
  return vv(c, 1, N, src1, src1Offset, inca, src2, src2Offset, incb, nullptr, 0, 0, dst,
            dstOffset, incc, "subvv");
}

int tns_hip_mulvv(tns_ctx* c, int64_t N, const float* src1, int64_t src1Offset, int64_t inca,
                  const float* src2, int64_t src2Offset, int64_t incb, float* dst,
                  int64_t dstOffset, int64_t incc) {
  return vv(c, 2, N, src1, src1Offset, inca, src2, src2Offset, incb, nullptr, 0, 0, dst,
            dstOffset, incc, "mulvv");
}

int tns_hip_fmavv(tns_ctx* c, int64_t N, const float* src1, int64_t src1Offset, int64_t inca,
                  const float* src2, int64_t src2Offset, int64_t incb, const float* src3,
                  int64_t src3Offset, int64_t incc, float* dst, int64_t dstOffset,
                  int64_t incd) {
  return vv(c, 3, N, src1, src1Offset, inca, src2, src2Offset, incb, src3, src3Offset, incc, dst,
            dstOffset, incd, "fmavv");
}

int tns_hip_fmavss(tns_ctx* c, int64_t N, const float* src, int64_t offset, float scalar,
                   float bias, float* dst) {
  if (int r = check_ops(c, {span(dst ? dst + offset : nullptr, N)},
                        {span(src ? src + offset : nullptr, N)}))
    return r;
  if (N < 0 || (N > 0 && (!src || !dst))) return set_error(TNS_ERR_ARG, "fmavss: bad args");
  return hip_status(launch_fmavss(N, src + offset, scalar, bias, dst + offset, c->stream),
                    "fmavss");
}

int tns_hip_inverse_sqrt(tns_ctx* c, int64_t N, float alpha, const float* src, float* dst,
                         int64_t stride, int64_t offset) {
  (void)alpha;  // unused by the reference kernel too
  if (int r = check_ops(c, {span(dst ? dst + offset : nullptr, N, stride)},
                        {span(src ? src + offset : nullptr, N, stride)}))
    return r;
  if (N < 0 || stride < 1 || (N > 0 && (!src || !dst)))
    return set_error(TNS_ERR_ARG, "inverseSqrt: bad args");
  return hip_status(launch_inverse_sqrt(N, src + offset, dst + offset, stride, c->stream),
                    "inverseSqrt");
}

int tns_hip_sgemm_strided_batched_multi(const int32_t* devices, int32_t n, uint8_t transA,
                                        uint8_t transB, int64_t M, int64_t N, int64_t K,
                                        float alpha, const float* A, int64_t lda,
                                        int64_t strideA, const float* B, int64_t ldb,
                                        int64_t strideB, float beta, float* C, int64_t ldc,
                                        int64_t strideC, int64_t batchCount) {
  if (!devices || n <= 0) return set_error(TNS_ERR_ARG, "sgemm_multi: no devices");
  const int nd = tns_device_count();
  for (int i = 0; i < n; ++i)
    if (devices[i] < 0 || devices[i] >= nd)
      return set_error(TNS_ERR_ARG, "sgemm_multi: device %d out of range [0,%d)", devices[i], nd);
  if (M < 0 || N < 0 || K < 0 || batchCount < 0)
    return set_error(TNS_ERR_ARG, "sgemm_multi: negative dimension");
  if (M == 0 || N == 0 || batchCount == 0) return TNS_OK;
  if (!C || (K > 0 && (!A || !B))) return set_error(TNS_ERR_ARG, "sgemm_multi: null operand");
  HostGemm g{transA != 0, transB != 0, M, N, K, alpha, beta, A, lda, strideA, B, ldb, strideB,
             C, ldc, strideC, batchCount};
  return multi_host_gemm(devices, n, g);
}

int tns_set_op_devices(const int32_t* devices, int32_t n) {
  const int nd = tns_device_count();
  for (int i = 0; i < n; ++i)
    if (!devices || devices[i] < 0 || devices[i] >= nd)
      return set_error(TNS_ERR_ARG, "set_op_devices: bad device list");
  std::lock_guard<std::mutex> lk(g_op_devices_mu);
  g_op_devices.assign(devices, devices + (n > 0 ? n : 0));
  return TNS_OK;
}

int tns_hip_yolo_forward(tns_ctx* c, int64_t batch, int64_t anchors, int64_t classes, int64_t hw,
                         const float* in, float* out) {
  {
    const int64_t n = batch * anchors * (classes + 5) * hw;
    if (int r = check_ops(c, {span(out, n)}, {span(in, n)})) return r;
  }
  if (batch < 0 || anchors < 0 || classes < 0 || hw < 0 ||
      (batch * anchors * hw > 0 && (!in || !out)))
    return set_error(TNS_ERR_ARG, "yolo: bad args");
  return hip_status(launch_yolo(batch, (int)anchors, (int)classes, hw, in, out, c->stream), "yolo");
}

int tns_hip_yolo_loss(tns_ctx* c, int64_t batch, int64_t anchors, int64_t classes, int64_t h,
                      int64_t w, int64_t total, const int64_t* mask, const float* biases,
                      int64_t maxBoxes, int64_t netW, int64_t netH, float ignoreThresh,
                      float truthThresh, float iouThresh, float iouNormalizer, float objNormalizer,
                      float* output, const float* truth, float* delta, float* cost, float* stats,
                      int64_t* counters) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (batch < 0 || anchors < 0 || classes < 0 || h < 0 || w < 0 || total < 0 || netW < 1 ||
      netH < 1)
    return set_error(TNS_ERR_ARG, "yolo loss: negative size, or a network extent below 1");
  if (maxBoxes < 1 || maxBoxes > kYoloMaxBoxes)
    return set_error(TNS_ERR_ARG, "yolo loss: maxBoxes %lld outside [1, %d]", (long long)maxBoxes,
                     kYoloMaxBoxes);
  if (anchors > kYoloMaxAnchors || total > kYoloMaxAnchors)
    return set_error(TNS_ERR_ARG, "yolo loss: more than %d anchors", kYoloMaxAnchors);
  const int64_t lim = 0x3fffffff;
  if (batch > 65535 || classes > lim || h > lim || w > lim || netW > (1 << 24) ||
      netH > (1 << 24) || h * w > lim || batch * anchors > lim ||
      batch * anchors * (classes + 5) > 0x7fff0000 / std::max<int64_t>(h * w, 1))
    return set_error(TNS_ERR_ARG, "yolo loss: batch beyond 65535, or a buffer beyond 2^31 elements");
  if (!output || !truth || !delta || !cost || !counters || (anchors > 0 && !mask) ||
      (total > 0 && !biases))
    return set_error(TNS_ERR_ARG, "yolo loss: null operand");
  YoloLossParams p{};
  for (int64_t i = 0; i < anchors; ++i) {
    if (mask[i] < 0 || mask[i] >= total)
      return set_error(TNS_ERR_ARG, "yolo loss: mask[%lld] = %lld outside [0, %lld)", (long long)i,
                       (long long)mask[i], (long long)total);
    p.mask[i] = (int)mask[i];
  }
  for (int64_t i = 0; i < 2 * total; ++i) p.biases[i] = biases[i];
  p.batch = (int)batch, p.n = (int)anchors, p.classes = (int)classes, p.h = (int)h, p.w = (int)w;
  p.total = (int)total, p.maxBoxes = (int)maxBoxes, p.netW = (int)netW, p.netH = (int)netH;
  p.ignoreThresh = ignoreThresh, p.truthThresh = truthThresh, p.iouThresh = iouThresh;
  p.iouNormalizer = iouNormalizer, p.objNormalizer = objNormalizer;
  const int64_t n = batch * anchors * (classes + 5) * h * w;
  if (int r = check_ops(c,
                        {span(delta, n), span(output, n), span(cost, 1), span(stats, 2 * batch),
                         span(reinterpret_cast<float*>(counters), 4)},
                        {span(truth, batch * maxBoxes * 6)}))
    return r;
  if (n == 0) {  // nothing to sum, no truth to count
    if (hipError_t e = launch_fill(1, cost, 0.0f, 1, c->stream); e != hipSuccess)
      return hip_status(e, "yolo loss");
    return hip_status(stats ? launch_fill(2 * batch, stats, 0.0f, 1, c->stream) : hipSuccess,
                      "yolo loss");
  }
  float* scratch = nullptr;
  if (int r = ensure_scratch(c, SLOT_YOLO, yolo_loss_scratch_floats(n), &scratch)) return r;
  return hip_status(launch_yolo_loss(p, output, truth, delta, cost, stats,
                                     reinterpret_cast<unsigned long long*>(counters), scratch,
                                     c->stream),
                    "yolo loss");
}

int tns_hip_yolo_detections(tns_ctx* c, int64_t batch, int64_t anchors, int64_t classes, int64_t h,
                            int64_t w, int64_t total, const int64_t* mask, const float* biases,
                            int64_t netW, int64_t netH, int64_t imW, int64_t imH, float thresh,
                            int32_t relative, int32_t letter, const float* output,
                            int64_t capacity, int64_t* counts, float* boxes, float* objectness,
                            float* probs) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (batch < 0 || anchors < 0 || classes < 0 || h < 0 || w < 0 || total < 0 || netW < 1 ||
      netH < 1 || imW < 1 || imH < 1)
    return set_error(TNS_ERR_ARG,
                     "yolo detections: negative size, or a network / image extent below 1");
  if (capacity < 1 || capacity > kDetMaxCapacity)
    return set_error(TNS_ERR_ARG, "yolo detections: capacity %lld outside [1, %d]",
                     (long long)capacity, kDetMaxCapacity);
  if (anchors > kYoloMaxAnchors || total > kYoloMaxAnchors)
    return set_error(TNS_ERR_ARG, "yolo detections: more than %d anchors", kYoloMaxAnchors);
  const int64_t lim = 0x3fffffff;
  if (batch > 65535 || classes > lim || h > lim || w > lim || netW > (1 << 24) ||
      netH > (1 << 24) || imW > (1 << 24) || imH > (1 << 24) || h * w > lim ||
      h * w * anchors > lim || batch * anchors > lim ||
      batch * anchors * (classes + 5) > 0x7fff0000 / std::max<int64_t>(h * w, 1) ||
      batch * capacity > 0x7fff0000 / std::max<int64_t>(classes, 4))
    return set_error(TNS_ERR_ARG,
                     "yolo detections: batch beyond 65535, an extent beyond 2^24, or a buffer "
                     "beyond 2^31 elements");
  const bool work = batch > 0 && anchors > 0 && h * w > 0;
  if (work && (!output || !counts || !boxes || !objectness || (classes > 0 && !probs) || !mask ||
               (total > 0 && !biases)))
    return set_error(TNS_ERR_ARG, "yolo detections: null operand");
  DetParams p{};
  for (int64_t i = 0; work && i < anchors; ++i) {
    if (mask[i] < 0 || mask[i] >= total)
      return set_error(TNS_ERR_ARG, "yolo detections: mask[%lld] = %lld outside [0, %lld)",
                       (long long)i, (long long)mask[i], (long long)total);
    p.mask[i] = (int)mask[i];
  }
  if (!work) return TNS_OK;
  for (int64_t i = 0; i < 2 * total; ++i) p.biases[i] = biases[i];
  p.batch = (int)batch, p.n = (int)anchors, p.classes = (int)classes, p.h = (int)h, p.w = (int)w;
  p.netW = (int)netW, p.netH = (int)netH, p.imW = (int)imW, p.imH = (int)imH;
  p.relative = relative != 0, p.letter = letter != 0, p.capacity = (int)capacity;
  p.thresh = thresh;
  if (int r = check_ops(c,
                        {span(boxes, batch * capacity * 4), span(objectness, batch * capacity),
                         span(probs, batch * capacity * classes),
                         span(reinterpret_cast<float*>(counts), 2 * batch)},
                        {span(output, batch * anchors * (classes + 5) * h * w)}))
    return r;
  float* scratch = nullptr;
  if (int r = ensure_scratch(c, SLOT_YOLO, detections_scratch_floats(p), &scratch)) return r;
  return hip_status(launch_yolo_detections(p, output, counts, boxes, objectness, probs, scratch,
                                           c->stream),
                    "yolo detections");
}

int tns_hip_nms_sort(tns_ctx* c, int64_t batch, int64_t capacity, int64_t classes,
                     const int64_t* counts, const float* boxes, const float* objectness,
                     float* probs, float thresh) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (batch < 0 || classes < 0) return set_error(TNS_ERR_ARG, "nms sort: negative size");
  if (capacity < 1 || capacity > kDetMaxCapacity)
    return set_error(TNS_ERR_ARG, "nms sort: capacity %lld outside [1, %d]", (long long)capacity,
                     kDetMaxCapacity);
  if (batch > 65535 || classes > 0x3fffffff ||
      batch * capacity > 0x7fff0000 / std::max<int64_t>(classes, 4))
    return set_error(TNS_ERR_ARG,
                     "nms sort: batch beyond 65535, or a buffer beyond 2^31 elements");
  if (batch == 0 || classes == 0) return TNS_OK;
  if (!counts || !boxes || !objectness || !probs)
    return set_error(TNS_ERR_ARG, "nms sort: null operand");
  if (int r = check_ops(c, {span(probs, batch * capacity * classes)},
                        {span(boxes, batch * capacity * 4), span(objectness, batch * capacity),
                         span(reinterpret_cast<const float*>(counts), 2 * batch)}))
    return r;
  return hip_status(launch_nms_sort((int)batch, (int)capacity, (int)classes, counts, boxes,
                                    objectness, probs, thresh, c->stream),
                    "nms sort");
}

// TImageData.resize / letterBox / letterBoxEx (ntypes.pas:837-947) into the
// network input.  Not a TNNCuda method, hence tns_image_*; instead of a place
// in the hazard table the two entries join the side stream on every call
namespace {
int image_to_input(tns_ctx* c, bool bytes, int64_t count, const void* src, const int64_t* geom,
                   int64_t channels, int64_t pixelStride, int32_t tableKind, const float* table,
                   int64_t netW, int64_t netH, int32_t letter, float* dst, int64_t* placed) {
  if (int r = check_ctx(c)) return r;
  const int64_t lim = kImageMaxExtent;
  if (count < 0 || count > (1 << 20))
    return set_error(TNS_ERR_ARG, "image: count %lld outside [0, 2^20]", (long long)count);
  if (netW < 1 || netW > lim || netH < 1 || netH > lim)
    return set_error(TNS_ERR_ARG, "image: net input %lld x %lld outside [1, %lld]",
                     (long long)netW, (long long)netH, (long long)lim);
  if (bytes ? (channels < 1 || channels > 4 || pixelStride < channels || pixelStride > lim)
            : (channels < 1 || channels > 1024))
    return set_error(TNS_ERR_ARG, "image: channels %lld (bytes: 1..4, floats: 1..1024) or pixel "
                     "stride %lld", (long long)channels, (long long)pixelStride);
  if (bytes && (tableKind < 0 || tableKind > 2))
    return set_error(TNS_ERR_ARG, "image: table kind %d", (int)tableKind);
  if (count == 0) return TNS_OK;
  if (!src || !geom || !dst || (bytes && tableKind == 2 && !table))
    return set_error(TNS_ERR_ARG, "image: null operand");
  std::vector<ImageGeom> gs((size_t)count);
  for (int64_t i = 0; i < count; ++i) {
    const int64_t off = geom[4 * i], w = geom[4 * i + 1], h = geom[4 * i + 2], rs = geom[4 * i + 3];
    if (off < 0 || w < 1 || w > lim || h < 1 || h > lim || rs < w * (bytes ? pixelStride : 1))
      return set_error(TNS_ERR_ARG, "image %lld: offset %lld, %lld x %lld outside [1, %lld], or "
                       "row stride %lld shorter than a row", (long long)i, (long long)off,
                       (long long)w, (long long)h, (long long)lim, (long long)rs);
    int64_t nw = netW, nh = netH;
    if (letter) {
      if (netW * h < netH * w)  // (aWidth / self.w) < (aHeight / self.h), exactly
        nh = h * netW / w;
      else
        nw = w * netH / h;
    }
    if (nw < 2 || nh < 2)  // the reference divides by aWidth-1, aHeight-1
      return set_error(TNS_ERR_ARG, "image %lld: resize target %lld x %lld below 2",
                       (long long)i, (long long)nw, (long long)nh);
    ImageGeom& g = gs[(size_t)i];
    g.off = off, g.rs = rs, g.w = (int)w, g.h = (int)h, g.nw = (int)nw, g.nh = (int)nh;
    g.dx = (int)((netW - nw) / 2), g.dy = (int)((netH - nh) / 2);
    // integer / integer is a real, stored to a single: one rounding of the
    // double quotient gives the same value for operands below 2^24
    g.ws = (float)((double)(w - 1) / (double)(nw - 1));
    g.hs = (float)((double)(h - 1) / (double)(nh - 1));
  }
  float tab[256] = {};
  for (int b = 0; bytes && b < 256; ++b)
    tab[b] = tableKind == 2   ? table[b]
             : tableKind == 1 ? (float)((double)b / 255.0)              // p.r / $ff
                              : (float)((double)(b * 257) / 65280.0);   // TFPColor word / $ff00
  for (int64_t i = 0; placed && i < count; ++i) {
    const ImageGeom& g = gs[(size_t)i];
    placed[4 * i] = g.nw, placed[4 * i + 1] = g.nh, placed[4 * i + 2] = g.dx;
    placed[4 * i + 3] = g.dy;
  }
  return hip_status(launch_image_to_input(bytes, gs.data(), count, src, (int)channels,
                                          (int)pixelStride, tab, (int)netW, (int)netH, dst,
                                          c->stream),
                    "image to input");
}
}  // namespace

int tns_image_bytes_to_input(tns_ctx* c, int64_t count, const uint8_t* src, const int64_t* geom,
                             int64_t channels, int64_t pixelStride, int32_t tableKind,
                             const float* table, int64_t netW, int64_t netH, int32_t letter,
                             float* dst, int64_t* placed) {
  return image_to_input(c, true, count, src, geom, channels, pixelStride, tableKind, table, netW,
                        netH, letter, dst, placed);
}

int tns_image_floats_to_input(tns_ctx* c, int64_t count, const float* src, const int64_t* geom,
                              int64_t channels, int64_t netW, int64_t netH, int32_t letter,
                              float* dst, int64_t* placed) {
  return image_to_input(c, false, count, src, geom, channels, 1, 0, nullptr, netW, netH, letter,
                        dst, placed);
}

// TNNCuda.forwardMaxPool / backwardMaxPool (nncuda.pas:132-133) and the local
// average pool over the same geometry
namespace {
// TMaxPoolLayer.Create's shapes (nMaxPoolLayer.pas:107-109) restated and held
// against the caller's; avg: no window without an in-range tap (the reference
// divides by a zero counter there).  *planes = aBatch*outC, *nin / *nout the
// whole buffers' element counts.
int pool_geom(const char* what, bool avg, int64_t aBatch, int64_t outC, int64_t outH, int64_t outW,
              int64_t c, int64_t h, int64_t w, int64_t sx, int64_t sy, int64_t padding,
              int64_t size, PoolGeom* g, int64_t* planes, int64_t* nin, int64_t* nout) {
  const int64_t lim = 0x3fffffff;
  if (aBatch < 0 || outC < 0 || outH < 0 || outW < 0 || c < 0 || h < 0 || w < 0 || size < 1 ||
      sx < 1 || sy < 1 || padding < 0)
    return set_error(TNS_ERR_ARG, "%s: negative size, or kernelSize / stride below 1", what);
  if (aBatch > lim || outC > lim || h > lim || w > lim || size > lim || sx > lim || sy > lim ||
      padding > lim)
    return set_error(TNS_ERR_ARG, "%s: dimension beyond 2^30", what);
  if (outC != c) return set_error(TNS_ERR_ARG, "%s: outC %lld != c %lld", what, (long long)outC,
                                  (long long)c);
  if (h + padding < size || w + padding < size)
    return set_error(TNS_ERR_ARG, "%s: kernelSize %lld exceeds the padded input", what,
                     (long long)size);
  const int64_t oh = (h + padding - size) / sy + 1, ow = (w + padding - size) / sx + 1;
  if (outH != oh || outW != ow)
    return set_error(TNS_ERR_ARG, "%s: output %lldx%lld, the geometry gives %lldx%lld", what,
                     (long long)outH, (long long)outW, (long long)oh, (long long)ow);
  if (h * w > 0x7fffffff || oh * ow > 0x7fffffff)
    return set_error(TNS_ERR_ARG, "%s: plane beyond 2^31 elements", what);
  const int64_t plane = std::max<int64_t>(std::max(h * w, oh * ow), 1);
  if (aBatch * outC > INT64_MAX / 8 / plane)
    return set_error(TNS_ERR_ARG, "%s: buffer beyond 2^63 bytes", what);
  const int64_t off = -(padding / 2);
  if (avg && (off + size - 1 < 0 || off + (oh - 1) * sy > h - 1 || off + (ow - 1) * sx > w - 1))
    return set_error(TNS_ERR_ARG, "%s: a window has no tap inside the input", what);
  *g = PoolGeom{(int)h, (int)w, (int)oh, (int)ow, (int)size, (int)sx, (int)sy, (int)off};
  *planes = aBatch * outC;
  *nin = *planes * h * w;
  *nout = *planes * oh * ow;
  return TNS_OK;
}
}  // namespace

int tns_hip_maxpool_forward(tns_ctx* c, int64_t aBatch, int64_t outC, int64_t outH, int64_t outW,
                            const float* input, int64_t ch, int64_t h, int64_t w,
                            int64_t stride_x, int64_t stride_y, int64_t padding,
                            int64_t kernelSize, int64_t* indexes, float* output) {
  PoolGeom g;
  int64_t planes, nin, nout;
  if (int r = pool_geom("maxpool forward", false, aBatch, outC, outH, outW, ch, h, w, stride_x,
                        stride_y, padding, kernelSize, &g, &planes, &nin, &nout))
    return r;
  if (nout > 0 && (!output || (nin > 0 && !input)))
    return set_error(TNS_ERR_ARG, "maxpool forward: null operand");
  // (the int64 indexes' byte extent: two floats per index)
  if (int r = check_ops(c, {span(output, nout), span(reinterpret_cast<float*>(indexes), 2 * nout)},
                        {span(input, nin)}))
    return r;
  return hip_status(launch_maxpool_forward(planes, g, input, output, indexes, c->stream),
                    "maxpool forward");
}

int tns_hip_maxpool_backward(tns_ctx* c, int64_t aBatch, int64_t outC, int64_t outH, int64_t outW,
                             float* output, const int64_t* indexes, const float* delta, int64_t h,
                             int64_t w, int64_t stride_x, int64_t stride_y, int64_t padding,
                             int64_t kernelSize) {
  PoolGeom g;
  int64_t planes, nin, nout;
  if (int r = pool_geom("maxpool backward", false, aBatch, outC, outH, outW, outC, h, w, stride_x,
                        stride_y, padding, kernelSize, &g, &planes, &nin, &nout))
    return r;
  if (nout > 0 && nin > 0 && (!output || !indexes || !delta))
    return set_error(TNS_ERR_ARG, "maxpool backward: null operand");
  if (int r = check_ops(c, {span(output, nin)},
                        {span(reinterpret_cast<const float*>(indexes), 2 * nout),
                         span(delta, nout)}))
    return r;
  return hip_status(launch_maxpool_backward(planes, g, output, indexes, delta, c->stream),
                    "maxpool backward");
}

int tns_hip_avgpool_forward(tns_ctx* c, int64_t aBatch, int64_t outC, int64_t outH, int64_t outW,
                            const float* input, int64_t ch, int64_t h, int64_t w,
                            int64_t stride_x, int64_t stride_y, int64_t padding,
                            int64_t kernelSize, float* output) {
  PoolGeom g;
  int64_t planes, nin, nout;
  if (int r = pool_geom("avgpool forward", true, aBatch, outC, outH, outW, ch, h, w, stride_x,
                        stride_y, padding, kernelSize, &g, &planes, &nin, &nout))
    return r;
  if (nout > 0 && (!output || !input))
    return set_error(TNS_ERR_ARG, "avgpool forward: null operand");
  if (int r = check_ops(c, {span(output, nout)}, {span(input, nin)})) return r;
  return hip_status(launch_avgpool_forward(planes, g, input, output, c->stream),
                    "avgpool forward");
}

int tns_hip_avgpool_backward(tns_ctx* c, int64_t aBatch, int64_t outC, int64_t outH, int64_t outW,
                             float* output, const float* delta, int64_t h, int64_t w,
                             int64_t stride_x, int64_t stride_y, int64_t padding,
                             int64_t kernelSize) {
  PoolGeom g;
  int64_t planes, nin, nout;
  if (int r = pool_geom("avgpool backward", true, aBatch, outC, outH, outW, outC, h, w, stride_x,
                        stride_y, padding, kernelSize, &g, &planes, &nin, &nout))
    return r;
  if (nout > 0 && (!output || !delta))
    return set_error(TNS_ERR_ARG, "avgpool backward: null operand");
  if (int r = check_ops(c, {span(output, nin)}, {span(delta, nout)})) return r;
  return hip_status(launch_avgpool_backward(planes, g, output, delta, c->stream),
                    "avgpool backward");
}

// TAvgPoolLayer.forward / backward (navgpoollayer.pas:60-108), which the
// reference runs on the CPU: not a TNNCuda method, hence no tns_hip_ prefix;
// like the tns_image_* entries the two join the side stream on every call
// instead of taking a place in the hazard table
namespace {
// small [planes] is written from (forward) or read into (backward) big
// [planes][n]; *work: there is something to do
int global_avg_args(tns_ctx* c, const char* what, int64_t planes, int64_t n, const float* small,
                    const float* big, bool* work) {
  if (int r = check_ctx(c)) return r;
  *work = false;
  if (planes < 0 || n < 0)
    return set_error(TNS_ERR_ARG, "%s: negative size (planes %lld, n %lld)", what,
                     (long long)planes, (long long)n);
  if (n > (1 << 24))  // float(n) must be exact
    return set_error(TNS_ERR_ARG, "%s: n %lld beyond 2^24", what, (long long)n);
  if (planes == 0 || n == 0) return TNS_OK;
  if (planes > INT64_MAX / 8 / n)
    return set_error(TNS_ERR_ARG, "%s: buffer beyond 2^63 bytes", what);
  if (!small || !big) return set_error(TNS_ERR_ARG, "%s: null operand", what);
  const Span a = span(small, planes), b = span(big, planes * n);
  if (a.lo < b.hi && b.lo < a.hi)
    return set_error(TNS_ERR_ARG, "%s: the operands overlap", what);
  *work = true;
  return TNS_OK;
}
}  // namespace

int tns_pool_global_avg_forward(tns_ctx* c, int64_t planes, int64_t n, const float* input,
                                float* output) {
  bool work;
  if (int r = global_avg_args(c, "global avgpool forward", planes, n, output, input, &work))
    return r;
  if (!work) return TNS_OK;
  return hip_status(launch_global_avgpool_forward(planes, n, input, output, c->stream),
                    "global avgpool forward");
}

int tns_pool_global_avg_backward(tns_ctx* c, int64_t planes, int64_t n, const float* delta,
                                 float* stateDelta) {
  bool work;
  if (int r = global_avg_args(c, "global avgpool backward", planes, n, delta, stateDelta, &work))
    return r;
  if (!work) return TNS_OK;
  return hip_status(launch_global_avgpool_backward(planes, n, delta, stateDelta, c->stream),
                    "global avgpool backward");
}

// ---- dropout / loss heads (heads.hip) -------------------------------------------
namespace {

// src == dst exactly is the reference's in-place call; any other meeting of
// the three operands would make a result depend on the thread order
int dropout_operands(const char* what, int64_t N, const float* src, const float* rnd,
                     const float* dst) {
  if (N < 0) return set_error(TNS_ERR_ARG, "%s: N = %lld", what, (long long)N);
  if (N == 0) return TNS_OK;
  if (!src || !rnd || !dst) return set_error(TNS_ERR_ARG, "%s: null operand", what);
  auto meet = [N](const float* a, const float* b) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)N * sizeof(float);
    return x < y + len && y < x + len;
  };
  if (meet(rnd, src) || meet(rnd, dst))
    return set_error(TNS_ERR_ARG, "%s: rnd overlaps src or dst", what);
  if (src != dst && meet(src, dst))
    return set_error(TNS_ERR_ARG, "%s: src and dst overlap without being the same buffer", what);
  return TNS_OK;
}

}  // namespace

int tns_hip_dropout_forward(tns_ctx* c, int64_t N, int64_t seed, float probability, float scale,
                            const float* src, float* rnd, float* dst) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (int r = dropout_operands("dropout forward", N, src, rnd, dst)) return r;
  if (seed < 0 || seed > (int64_t)0xFFFFFFFFll)
    return set_error(TNS_ERR_ARG, "dropout forward: seed %lld outside [0, 2^32)", (long long)seed);
  if (N == 0) return TNS_OK;
  if (int r = check_ops(c, {span(dst, N), span(rnd, N)}, {span(src, N)})) return r;
  return hip_status(launch_dropout_forward(N, (uint32_t)seed, probability, scale, src, rnd, dst,
                                           c->stream),
                    "dropout forward");
}

int tns_hip_dropout_backward(tns_ctx* c, int64_t N, float probability, float scale,
                             const float* src, const float* rnd, float* dst) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (int r = dropout_operands("dropout backward", N, src, rnd, dst)) return r;
  if (N == 0) return TNS_OK;
  if (int r = check_ops(c, {span(dst, N)}, {span(src, N), span(rnd, N)})) return r;
  return hip_status(launch_dropout_backward(N, probability, scale, src, rnd, dst, c->stream),
                    "dropout backward");
}

int tns_hip_cost_l2(tns_ctx* c, int64_t N, const float* pred, const float* truth, float* delta,
                    float* error) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (N < 0) return set_error(TNS_ERR_ARG, "costL2: N = %lld", (long long)N);
  if (N == 0) return TNS_OK;
  if (!pred || !truth || !delta || !error) return set_error(TNS_ERR_ARG, "costL2: null operand");
  if (int r = check_ops(c, {span(delta, N), span(error, N)}, {span(pred, N), span(truth, N)}))
    return r;
  return hip_status(launch_cost_l2(N, pred, truth, delta, error, c->stream), "costL2");
}

int tns_hip_cross_entropy_logistic(tns_ctx* c, int64_t N, const float* pred, const float* truth,
                                   float* delta, float* error) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (N < 0) return set_error(TNS_ERR_ARG, "crossEntropyLogistic: N = %lld", (long long)N);
  if (N == 0) return TNS_OK;
  if (!pred || !truth || !delta || !error)
    return set_error(TNS_ERR_ARG, "crossEntropyLogistic: null operand");
  if (int r = check_ops(c, {span(delta, N), span(error, N)}, {span(pred, N), span(truth, N)}))
    return r;
  return hip_status(launch_xent_logistic(N, pred, truth, delta, error, c->stream),
                    "crossEntropyLogistic");
}

namespace {

// the LSTM gate entries: no output may meet any other operand (an in / out
// operand is one operand); inputs may meet one another
static int lstm_operands(const char* what, int64_t N, std::initializer_list<const float*> in,
                  std::initializer_list<const float*> out,
                  std::initializer_list<const float*> optional_out) {
  if (N < 0) return set_error(TNS_ERR_ARG, "%s: N = %lld", what, (long long)N);
  if (N == 0) return TNS_OK;
  for (const float* p : in)
    if (!p) return set_error(TNS_ERR_ARG, "%s: null operand", what);
  for (const float* p : out)
    if (!p) return set_error(TNS_ERR_ARG, "%s: null operand", what);
  const uintptr_t len = (uintptr_t)N * sizeof(float);
  auto meet = [len](const float* a, const float* b) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + len && y < x + len;
  };
  std::vector<const float*> outs(out);
  outs.insert(outs.end(), optional_out.begin(), optional_out.end());
  for (size_t a = 0; a < outs.size(); ++a) {
    for (size_t b = a + 1; b < outs.size(); ++b)
      if (meet(outs[a], outs[b]))
        return set_error(TNS_ERR_ARG, "%s: two outputs overlap", what);
    for (const float* p : in)
      if (meet(outs[a], p))
        return set_error(TNS_ERR_ARG, "%s: an output overlaps an input", what);
  }
  return TNS_OK;
}

}  // namespace

int tns_hip_lstm_gates_forward(tns_ctx* c, int64_t N, const float* wf, const float* wi,
                               const float* wg, const float* wo, const float* uf,
                               const float* ui, const float* ug, const float* uo, float* c_state,
                               float* h_state, float* cell_slice, float* out_slice) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (int r = lstm_operands("lstmGatesForward", N, {wf, wi, wg, wo, uf, ui, ug, uo},
                            {c_state, h_state, cell_slice, out_slice}, {}))
    return r;
  if (N == 0) return TNS_OK;
  if (int r = check_ops(c,
                        {span(c_state, N), span(h_state, N), span(cell_slice, N),
                         span(out_slice, N)},
                        {span(wf, N), span(wi, N), span(wg, N), span(wo, N), span(uf, N),
                         span(ui, N), span(ug, N), span(uo, N)}))
    return r;
  const float* const w[4] = {wf, wi, wg, wo};
  const float* const u[4] = {uf, ui, ug, uo};
  return hip_status(
      launch_lstm_gates_forward(N, w, u, c_state, h_state, cell_slice, out_slice, c->stream),
      "lstmGatesForward");
}

int tns_hip_lstm_gates_backward(tns_ctx* c, int64_t N, const float* wf, const float* wi,
                                const float* wg, const float* wo, const float* uf,
                                const float* ui, const float* ug, const float* uo,
                                const float* cell_i, const float* cprev, const float* delta_i,
                                float* dc, float* dwf, float* dwi, float* dwg, float* dwo,
                                float* duf, float* dui, float* dug, float* duo) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (int r = lstm_operands("lstmGatesBackward", N,
                            {wf, wi, wg, wo, uf, ui, ug, uo, cell_i, cprev, delta_i},
                            {dc, dwf, dwi, dwg, dwo}, {duf, dui, dug, duo}))
    return r;
  if (N == 0) return TNS_OK;
  if (int r = check_ops(c,
                        {span(dc, N), span(dwf, N), span(dwi, N), span(dwg, N), span(dwo, N),
                         span(duf, N), span(dui, N), span(dug, N), span(duo, N)},
                        {span(wf, N), span(wi, N), span(wg, N), span(wo, N), span(uf, N),
                         span(ui, N), span(ug, N), span(uo, N), span(cell_i, N), span(cprev, N),
                         span(delta_i, N)}))
    return r;
  const float* const w[4] = {wf, wi, wg, wo};
  const float* const u[4] = {uf, ui, ug, uo};
  float* const dw[4] = {dwf, dwi, dwg, dwo};
  float* const du[4] = {duf, dui, dug, duo};
  return hip_status(launch_lstm_gates_backward(N, w, u, cell_i, cprev, delta_i, dc, dw, du,
                                               c->stream),
                    "lstmGatesBackward");
}

namespace {

// the RNN step entries: operands as (pointer, floats); the first n_out are
// written.  No output may meet any other operand (an in / out operand is one
// operand; null operands meet nothing); inputs may meet one another
struct RnnOp {
  const float* p;
  int64_t n;
};
int rnn_overlap(const char* what, std::initializer_list<RnnOp> ops, size_t n_out) {
  auto meet = [](const RnnOp& a, const RnnOp& b) {
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return a.p && b.p && x < y + (uintptr_t)b.n * sizeof(float) &&
           y < x + (uintptr_t)a.n * sizeof(float);
  };
  const RnnOp* o = ops.begin();
  for (size_t a = 0; a < n_out; ++a)
    for (size_t b = 0; b < ops.size(); ++b)
      if (b != a && (b > a || b >= n_out) && meet(o[a], o[b]))
        return set_error(TNS_ERR_ARG, "%s: an output overlaps another operand", what);
  return TNS_OK;
}

}  // namespace

int tns_hip_rnn_state_forward(tns_ctx* c, int64_t N, int64_t H, float* in_slice,
                              const float* in_bias, int32_t in_act, float* self_slice,
                              const float* self_bias, int32_t self_act, const float* state_prev,
                              float* state_next) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (N < 0 || H < 1)
    return set_error(TNS_ERR_ARG, "rnnStateForward: N = %lld, H = %lld", (long long)N,
                     (long long)H);
  if (!act_supported(in_act) || !act_supported(self_act))
    return set_error(TNS_ERR_UNSUPPORTED, "rnnStateForward: activation %d / %d not implemented",
                     in_act, self_act);
  if (N == 0) return TNS_OK;
  if (!in_slice || !self_slice || !state_next)
    return set_error(TNS_ERR_ARG, "rnnStateForward: null operand");
  // state_prev == state_next is the in-place call (inference, j = i)
  const float* prev = state_prev == state_next ? nullptr : state_prev;
  if (int r = rnn_overlap("rnnStateForward",
                          {{in_slice, N}, {self_slice, N}, {state_next, N}, {prev, N},
                           {in_bias, H}, {self_bias, H}},
                          3))
    return r;
  if (int r = check_ops(c, {span(in_slice, N), span(self_slice, N), span(state_next, N)},
                        {span(state_prev, N), span(in_bias, H), span(self_bias, H)}))
    return r;
  return hip_status(launch_rnn_state_forward(N, H, in_slice, in_bias, in_act, self_slice,
                                             self_bias, self_act, state_prev, state_next,
                                             c->stream),
                    "rnnStateForward");
}

int tns_hip_rnn_delta_backward(tns_ctx* c, int64_t N, float* delta, const float* out, int32_t act,
                               float* delta2, const float* out2, int32_t act2) {
  if (!c) return set_error(TNS_ERR_ARG, "null tns_ctx");
  if (N < 0) return set_error(TNS_ERR_ARG, "rnnDeltaBackward: N = %lld", (long long)N);
  if (!act_supported(act) || (delta2 && !act_supported(act2)))
    return set_error(TNS_ERR_UNSUPPORTED, "rnnDeltaBackward: derivative %d / %d not implemented",
                     act, act2);
  if (N == 0) return TNS_OK;
  if (!delta || !out || (delta2 && !out2))
    return set_error(TNS_ERR_ARG, "rnnDeltaBackward: null operand");
  if (int r = rnn_overlap("rnnDeltaBackward",
                          {{delta, N}, {delta2, N}, {out, N}, {delta2 ? out2 : nullptr, N}}, 2))
    return r;
  if (int r = check_ops(c, {span(delta, N), span(delta2, N)},
                        {span(out, N), span(delta2 ? out2 : nullptr, N)}))
    return r;
  return hip_status(launch_rnn_delta_backward(N, delta, out, act, delta2, out2, act2, c->stream),
                    "rnnDeltaBackward");
}

int tns_hip_clamp(tns_ctx* c, int64_t N, float alpha, const float* src, float* dst,
                  int64_t stride, int64_t offset) {
  if (int r = check_ops(c, {span(dst ? dst + offset : nullptr, N, stride)},
                        {span(src ? src + offset : nullptr, N, stride)}))
    return r;
  if (N < 0 || stride < 1 || (N > 0 && (!src || !dst)))
    return set_error(TNS_ERR_ARG, "clamp: bad args");
  return hip_status(launch_clamp(N, alpha, src + offset, dst + offset, stride, c->stream),
                    "clamp");
}

// ---- batch norm / softmax ------------------------------------------------------
namespace {
int blocks_of(int64_t total, int64_t channels, int64_t groups, int64_t* bs, const char* what) {
  if (channels <= 0 || groups <= 0 || total < 0 || total % (channels * groups) != 0)
    return set_error(TNS_ERR_ARG, "%s: sizes do not align (total=%lld channels=%lld groups=%lld)",
                     what, (long long)total, (long long)channels, (long long)groups);
  *bs = total / (channels * groups);
  return TNS_OK;
}
}  // namespace

int tns_hip_means_and_vars(tns_ctx* c, int64_t srcSize, int64_t dstSize, int64_t groups,
                           const float* src, int64_t offset, float* means, float* vars) {
  if (int r = check_ops(c, {span(means, dstSize), span(vars, dstSize)},
                        {span(src ? src + offset : nullptr, srcSize)}))
    return r;
  int64_t bs;
  if (int r = blocks_of(srcSize, dstSize, groups, &bs, "meansAndVars")) return r;
  if (!src || !means || !vars) return set_error(TNS_ERR_ARG, "meansAndVars: null pointer");
  float* part;
  if (int r = ensure_scratch(c, SLOT_BN, 2 * groups * dstSize, &part)) return r;
  return hip_status(launch_means_vars(src + offset, groups, dstSize, bs, means, vars,
                                      (int)g_opt.srss_quirk, part, c->stream),
                    "meansAndVars");
}

int tns_hip_means(tns_ctx* c, int64_t srcSize, int64_t dstSize, int64_t groups,
                  const float* src, int64_t offset, float* means) {
  if (int r = check_ops(c, {span(means, dstSize)}, {span(src ? src + offset : nullptr, srcSize)}))
    return r;
  int64_t bs;
  if (int r = blocks_of(srcSize, dstSize, groups, &bs, "means")) return r;
  if (!src || !means) return set_error(TNS_ERR_ARG, "means: null pointer");
  float* part;
  if (int r = ensure_scratch(c, SLOT_BN, 2 * groups * dstSize, &part)) return r;
  return hip_status(launch_means_vars(src + offset, groups, dstSize, bs, means, nullptr,
                                      (int)g_opt.srss_quirk, part, c->stream, 1),
                    "means");
}

int tns_hip_variances(tns_ctx* c, int64_t srcSize, int64_t dstSize, int64_t groups,
                      const float* src, int64_t offset, const float* means, float* vars) {
  if (int r = check_ops(c, {span(vars, dstSize)},
                        {span(src ? src + offset : nullptr, srcSize), span(means, dstSize)}))
    return r;
  int64_t bs;
  if (int r = blocks_of(srcSize, dstSize, groups, &bs, "variances")) return r;
  if (!src || !means || !vars) return set_error(TNS_ERR_ARG, "variances: null pointer");
  float* part;
  if (int r = ensure_scratch(c, SLOT_BN, 2 * groups * dstSize, &part)) return r;
  return hip_status(launch_means_vars(src + offset, groups, dstSize, bs,
                                      const_cast<float*>(means), vars, (int)g_opt.srss_quirk, part,
                                      c->stream, 2),
                    "variances");
}

int tns_hip_normalize(tns_ctx* c, int64_t srcSize, int64_t dstSize, int64_t groups,
                      const float* means, int64_t meansStride, const float* vars,
                      int64_t varsStride, float* dst, int64_t dstOffset) {
  if (int r = check_ops(c, {span(dst ? dst + dstOffset : nullptr, dstSize)},
                        {span(means, srcSize, meansStride), span(vars, srcSize, varsStride)}))
    return r;
  int64_t bs;
  if (int r = blocks_of(dstSize, srcSize, groups, &bs, "normalize")) return r;
  if (!dst || !means || !vars) return set_error(TNS_ERR_ARG, "normalize: null pointer");
  return hip_status(launch_normalize(dst + dstOffset, groups, srcSize, bs, means, meansStride,
                                     vars, varsStride, c->stream),
                    "normalize");
}

int tns_hip_forward_scale(tns_ctx* c, int64_t dstSize, float* dst, int64_t offset,
                          int64_t scaleSize, const float* scale, int64_t incb, int64_t batch) {
  return tns_hip_forward_scale_add(c, dstSize, dst, offset, scaleSize, scale, nullptr, incb,
                                   batch);
}

int tns_hip_forward_scale_add(tns_ctx* c, int64_t dstSize, float* dst, int64_t offset,
                              int64_t scaleSize, const float* scales, const float* biases,
                              int64_t incb, int64_t batch) {
  if (int r = check_ops(c, {span(dst ? dst + offset : nullptr, dstSize)},
                        {span(scales, scaleSize, incb), span(biases, scaleSize, incb)}))
    return r;
  if (incb < 1) return set_error(TNS_ERR_ARG, "forwardScale: incb < 1");
  int64_t bs;
  if (int r = blocks_of(dstSize, scaleSize, batch, &bs, "forwardScale")) return r;
  if (!dst || !scales) return set_error(TNS_ERR_ARG, "forwardScale: null pointer");
  return hip_status(launch_scale_add(dst + offset, batch, scaleSize, bs, scales, biases, incb,
                                     c->stream),
                    "forwardScale");
}

int tns_hip_means_and_vars_delta(tns_ctx* c, int64_t srcSize, int64_t dstSize, int64_t groups,
                                 const float* delta, const float* x, int64_t offset,
                                 const float* mean, const float* variance, float* mean_delta,
                                 float* variance_delta) {
  if (int r = check_ops(c, {span(mean_delta, dstSize), span(variance_delta, dstSize)},
                        {span(delta ? delta + offset : nullptr, srcSize),
                         span(x ? x + offset : nullptr, srcSize), span(mean, dstSize),
                         span(variance, dstSize)}))
    return r;
  int64_t bs;
  if (int r = blocks_of(srcSize, dstSize, groups, &bs, "meansAndVarsDelta")) return r;
  if (!delta || !x || !mean || !variance || !mean_delta || !variance_delta)
    return set_error(TNS_ERR_ARG, "meansAndVarsDelta: null pointer");
  float* part;
  if (int r = ensure_scratch(c, SLOT_BN, 2 * groups * dstSize, &part)) return r;
  return hip_status(launch_mean_var_delta(delta + offset, x + offset, mean, variance, groups,
                                          dstSize, bs, mean_delta, variance_delta,
                                          (int)g_opt.srss_quirk, part, c->stream),
                    "meansAndVarsDelta");
}

int tns_hip_normalize_delta(tns_ctx* c, int64_t deltaSize, int64_t meanSize, int64_t groups,
                            float* delta, const float* x, int64_t offset, const float* mean,
                            const float* variance, const float* mean_delta,
                            const float* variance_delta) {
  if (int r = check_ops(c, {span(delta ? delta + offset : nullptr, deltaSize)},
                        {span(x ? x + offset : nullptr, deltaSize), span(mean, meanSize),
                         span(variance, meanSize), span(mean_delta, meanSize),
                         span(variance_delta, meanSize)}))
    return r;
  int64_t bs;
  if (int r = blocks_of(deltaSize, meanSize, groups, &bs, "normalizeDelta")) return r;
  if (!delta || !x || !mean || !variance || !mean_delta || !variance_delta)
    return set_error(TNS_ERR_ARG, "normalizeDelta: null pointer");
  return hip_status(launch_normalize_delta(x + offset, mean, variance, mean_delta,
                                           variance_delta, delta + offset, groups, meanSize, bs,
                                           c->stream),
                    "normalizeDelta");
}

int tns_hip_add_dots(tns_ctx* c, int64_t N, int64_t dstSize, int64_t groups, const float* src1,
                     const float* src2, int64_t srcOffset, float* dst) {
  if (int r = check_ops(c, {span(dst, dstSize)},
                        {span(src1 ? src1 + srcOffset : nullptr, N),
                         span(src2 ? src2 + srcOffset : nullptr, N)}))
    return r;
  int64_t bs;
  if (int r = blocks_of(N, dstSize, groups, &bs, "addDots")) return r;
  if (!dst || !src1 || !src2) return set_error(TNS_ERR_ARG, "addDots: null pointer");
  float* part;
  if (int r = ensure_scratch(c, SLOT_BN, 2 * groups * dstSize, &part)) return r;
  return hip_status(launch_add_dots(dst, src1 + srcOffset, src2 + srcOffset, groups, dstSize, bs,
                                    part, c->stream),
                    "addDots");
}

int tns_hip_softmax_batch(tns_ctx* c, int64_t N, const float* input, int64_t iOffset,
                          int64_t batch, int64_t batch_size, int64_t groups, int64_t group_size,
                          int64_t stride, float temp, float* output, int64_t oOffset) {
  // every (batch, group) row's n strided elements: the last one ends the extent
  const int64_t ext = (N > 0 && batch > 0 && groups > 0 && batch_size >= 0 && group_size >= 0 &&
                       stride >= 1)
                          ? (batch - 1) * batch_size + (groups - 1) * group_size +
                                (N - 1) * stride + 1
                          : 0;
  if (int r = check_ops(c, {span(output ? output + oOffset : nullptr, ext)},
                        {span(input ? input + iOffset : nullptr, ext)}))
    return r;
  if (!input || !output || N < 0 || stride < 1 || batch < 0 || groups < 0 || batch_size < 0 ||
      group_size < 0)
    return set_error(TNS_ERR_ARG, "softmaxBatch: bad args");
  return hip_status(launch_softmax_batch(N, input + iOffset, batch, batch_size, groups,
                                         group_size, stride, temp, output + oOffset, c->stream),
                    "softmaxBatch");
}

int tns_hip_cross_entropy_softmax(tns_ctx* c, int64_t N, const float* pred, const float* truth,
                                  float* delta, float* error) {
  if (int r = check_ops(c, {span(delta, N), span(error, N)}, {span(pred, N), span(truth, N)}))
    return r;
  if (!pred || !truth || !delta || !error) return set_error(TNS_ERR_ARG, "xent: null pointer");
  return hip_status(launch_xent_softmax(N, pred, truth, delta, error, c->stream), "xent");
}

int tns_hip_sum(tns_ctx* c, int64_t N, const float* src, int64_t offset, float* out) {
  if (int r = check_ops(c, {span(out, 1)}, {span(src ? src + offset : nullptr, N)})) return r;
  if (!src || !out || N < 0) return set_error(TNS_ERR_ARG, "sum: bad args");
  return hip_status(launch_vssum(N, src + offset, out, c->stream), "sum");
}

int64_t tns_mlp_buffer_floats(int32_t nlayers, const int64_t* widths, int32_t bn, int64_t batch) {
  if (nlayers <= 0 || nlayers > 32 || !widths) return -1;
  return mlp_buffer_floats(nlayers, widths, bn, batch);
}

int tns_hip_mlp_train_step(tns_ctx* c, int32_t nlayers, const int64_t* widths,
                           const int32_t* acts, int32_t bn, int64_t batch, const float* X,
                           const float* truth, float learningRate, float momentum, float decay,
                           float* buf, float* cost) {
  if (int r = check_ctx(c)) return r;
  if (nlayers <= 0 || nlayers > MLP_MAX_LAYERS || !widths || !acts || !X || !truth || !buf ||
      !cost)
    return set_error(TNS_ERR_ARG, "mlp_train_step: bad arguments");
  if (batch < 2) return set_error(TNS_ERR_ARG, "mlp_train_step: batch must be >= 2 (BN)");
  MlpArgs a;
  a.nlayers = nlayers;
  int64_t omax = 0;
  for (int l = 0; l <= nlayers; ++l) {
    if (widths[l] <= 0) return set_error(TNS_ERR_ARG, "mlp_train_step: width %d <= 0", l);
    a.widths[l] = widths[l];
    if (l > 0 && widths[l] > omax) omax = widths[l];
  }
  if (9 * batch * omax > 40960)
    return set_error(TNS_ERR_ARG, "mlp_train_step: 9*batch*max(width) exceeds LDS staging");
  // (the kernels index a layer's weights and activations with 32-bit ints)
  for (int l = 0; l < nlayers; ++l)
    if (widths[l] * widths[l + 1] > 0x7fffffffLL)
      return set_error(TNS_ERR_ARG, "mlp_train_step: layer %d has %lld weights (32-bit indexing)",
                       l, (long long)(widths[l] * widths[l + 1]));
  if (batch * widths[0] > 0x7fffffffLL)
    return set_error(TNS_ERR_ARG, "mlp_train_step: batch x input width exceeds 32-bit indexing");
  for (int l = 0; l < nlayers; ++l) {
    if (!act_supported(acts[l]))
      return set_error(TNS_ERR_UNSUPPORTED, "mlp_train_step: activation %d", acts[l]);
    a.acts[l] = acts[l];
  }
  a.bn = bn != 0;
  a.batch = batch;
  a.X = X;
  a.truth = truth;
  a.lr = learningRate;
  a.momentum = momentum;
  a.decay = decay;
  a.buf = buf;
  a.cost = cost;
  // layer 0's residue partials (8 x batch x widths[1]), handed from the
  // layer-0 forward launch to the fused one
  if (int r = ensure_scratch(c, SLOT_MLP, 8 * batch * widths[1], &a.l0part)) return r;
  return hip_status(launch_mlp_train_step(a, c->stream), "mlp_train_step");
}

int tns_gemm_variant_count(void) { return sgemm_variant_count(); }
int tns_sdot_chains_variant_count(void) { return sdot_chains_variant_count(); }
const char* tns_sdot_chains_variant_name(int32_t v) { return sdot_chains_variant_name(v); }
int tns_sdot_rc_variant_count(void) { return sdot_rc_variant_count(); }
const char* tns_sdot_rc_variant_name(int32_t v) { return sdot_rc_variant_name(v); }
const char* tns_gemm_variant_name(int32_t v) { return sgemm_variant_name(v); }

int tns_hip_gemm_variant(tns_ctx* c, int32_t variant, uint8_t transA, uint8_t transB, int64_t M,
                         int64_t N, int64_t K, float ALPHA, const float* A, int64_t aOffset,
                         int64_t lda, int64_t strideA, const float* B, int64_t bOffset,
                         int64_t ldb, int64_t strideB, float BETA, float* C, int64_t cOffset,
                         int64_t ldc, int64_t strideC, int64_t batchCount) {
  if (int r = check_ctx(c)) return r;
  if (variant >= sgemm_variant_count())
    return set_error(TNS_ERR_ARG, "gemm variant %d out of range", variant);
  return do_gemm(c, transA != 0, transB != 0, M, N, K, ALPHA, A ? A + aOffset : nullptr, lda,
                 strideA, B ? B + bOffset : nullptr, ldb, strideB, BETA,
                 C ? C + cOffset : nullptr, ldc, strideC, batchCount, EPI_NONE, nullptr, 0, false,
                 variant);
}

int tns_hip_set_telemetry(tns_ctx* c, int32_t enable) {
  if (int r = check_ctx(c)) return r;
  c->telemetry = enable != 0;
  if (c->telemetry)
    for (double& v : c->op_ms) v = 0.0;
  return TNS_OK;
}

double tns_hip_op_ms(tns_ctx* c, int32_t op) {
  if (!c || op < 0 || op >= TNS_OP_COUNT) return 0.0;
  return c->op_ms[op];
}

// ---- boundary A: host-pointer op-table drop-ins ------------------------------
// Each stages operands through the default context's scratch and returns when
// C (or col/im) holds the result.  No status channel exists in the Pascal
// pointer types, so failures go to tns_last_error() / the error hook.

void tns_cblas_sgemm_batch_strided(int32_t Layout, int32_t TransA, int32_t TransB, int64_t M,
                                   int64_t N, int64_t K, float alpha, const float* A, int64_t lda,
                                   int64_t strideA, const float* B, int64_t ldb, int64_t strideB,
                                   float beta, float* C, int64_t ldc, int64_t strideC,
                                   int64_t batch_size) {
  (void)Layout;  // ignored, as cblas_sgemm ignores Order (ntensors.pas:2231)
  if ((TransA != TNS_CblasNoTrans && TransA != TNS_CblasTrans) ||
      (TransB != TNS_CblasNoTrans && TransB != TNS_CblasTrans)) {
    set_error(TNS_ERR_ARG, "cblas_sgemm: bad transpose enum");
    return;
  }
  if (M <= 0 || N <= 0 || batch_size <= 0) return;
  HostGemm g{TransA == TNS_CblasTrans, TransB == TNS_CblasTrans, M, N, K, alpha, beta,
             A, lda, strideA, B, ldb, strideB, C, ldc, strideC, batch_size};
  {
    std::lock_guard<std::mutex> lk(g_op_devices_mu);
    if (g_op_devices.size() > 1) {  // tns_set_op_devices: spread over several GPUs
      multi_host_gemm(g_op_devices.data(), (int)g_op_devices.size(), g);
      return;
    }
  }
  tns_ctx* c = default_ctx();
  if (!c) return;
  host_gemm(c, g, nullptr, nullptr);
}

void tns_cblas_sgemm(int32_t Order, int32_t TransA, int32_t TransB, int64_t M, int64_t N,
                     int64_t K, float ALPHA, const float* A, int64_t lda, const float* B,
                     int64_t ldb, float BETA, float* C, int64_t ldc) {
  tns_cblas_sgemm_batch_strided(Order, TransA, TransB, M, N, K, ALPHA, A, lda, 0, B, ldb, 0,
                                BETA, C, ldc, 0, 1);
}

void tns_im2col_strided_batched(int64_t aChannels, int64_t aHeight, int64_t aWidth,
                                int64_t kernelHeight, int64_t kernelWidth, int64_t padHeight,
                                int64_t padWidth, int64_t strideY, int64_t strideX,
                                int64_t dilationY, int64_t dilationX, const float* im,
                                int64_t imStride, int64_t imOffset, float* col,
                                int64_t colStride, int64_t colOffset, int64_t batchCount) {
  tns_ctx* c = default_ctx();
  if (!c || batchCount <= 0) return;
  ConvGeom g = geom(aChannels, aHeight, aWidth, kernelHeight, kernelWidth, padHeight, padWidth,
                    strideY, strideX, dilationY, dilationX);
  if (check_geom(g) || g.oh <= 0 || g.ow <= 0) return;
  std::lock_guard<std::mutex> lk(c->mu);
  hipSetDevice(c->device);
  const int64_t imgElems = aChannels * aHeight * aWidth;
  const int64_t colElems = aChannels * kernelHeight * kernelWidth * g.oh * g.ow;
  // pack images/cols densely on the device; strides apply on the host side
  float *dIm = nullptr, *dCol = nullptr;
  if (ensure_scratch(c, 1, imgElems * batchCount, &dIm) ||
      ensure_scratch(c, 2, colElems * batchCount, &dCol))
    return;
  hipStream_t s = c->stream;
  for (int64_t b = 0; b < batchCount; ++b)
    if (hip_status(hipMemcpyAsync(dIm + b * imgElems, im + imOffset + b * imStride,
                                  imgElems * 4, hipMemcpyHostToDevice, s),
                   "H2D im"))
      return;
  {
    OpTimer t(c, TNS_OP_IM2COL);
    if (hip_status(launch_im2col(g, dIm, imgElems, dCol, colElems, batchCount, s), "im2col"))
      return;
  }
  for (int64_t b = 0; b < batchCount; ++b)
    if (hip_status(hipMemcpyAsync(col + colOffset + b * colStride, dCol + b * colElems,
                                  colElems * 4, hipMemcpyDeviceToHost, s),
                   "D2H col"))
      return;
  hip_status(hipStreamSynchronize(s), "sync");
}

void tns_im2col(int64_t aChannels, int64_t aHeight, int64_t aWidth, int64_t kernelHeight,
                int64_t kernelWidth, int64_t padHeight, int64_t padWidth, int64_t strideY,
                int64_t strideX, int64_t dilationY, int64_t dilationX, const float* inData,
                int64_t inOffset, float* outData, int64_t outOffset, uint8_t multiThread) {
  (void)multiThread;  // the device kernel is always parallel and race-free
  tns_im2col_strided_batched(aChannels, aHeight, aWidth, kernelHeight, kernelWidth, padHeight,
                             padWidth, strideY, strideX, dilationY, dilationX, inData, 0,
                             inOffset, outData, 0, outOffset, 1);
}

void tns_col2im_strided_batched(int64_t aChannels, int64_t aHeight, int64_t aWidth,
                                int64_t kernelHeight, int64_t kernelWidth, int64_t padHeight,
                                int64_t padWidth, int64_t strideY, int64_t strideX,
                                int64_t dilationY, int64_t dilationX, const float* inData,
                                int64_t inStride, int64_t inOffset, float* outData,
                                int64_t outStride, int64_t outOffset, int64_t batchCount) {
  tns_ctx* c = default_ctx();
  if (!c || batchCount <= 0) return;
  ConvGeom g = geom(aChannels, aHeight, aWidth, kernelHeight, kernelWidth, padHeight, padWidth,
                    strideY, strideX, dilationY, dilationX);
  if (check_geom(g) || g.oh <= 0 || g.ow <= 0) return;
  std::lock_guard<std::mutex> lk(c->mu);
  hipSetDevice(c->device);
  const int64_t imgElems = aChannels * aHeight * aWidth;
  const int64_t colElems = aChannels * kernelHeight * kernelWidth * g.oh * g.ow;
  float *dIm = nullptr, *dCol = nullptr;
  if (ensure_scratch(c, 1, imgElems * batchCount, &dIm) ||
      ensure_scratch(c, 2, colElems * batchCount, &dCol))
    return;
  hipStream_t s = c->stream;
  for (int64_t b = 0; b < batchCount; ++b) {
    if (hip_status(hipMemcpyAsync(dCol + b * colElems, inData + inOffset + b * inStride,
                                  colElems * 4, hipMemcpyHostToDevice, s),
                   "H2D col"))
      return;
    // col2im accumulates into the existing image (ntensors.pas:11703)
    if (hip_status(hipMemcpyAsync(dIm + b * imgElems, outData + outOffset + b * outStride,
                                  imgElems * 4, hipMemcpyHostToDevice, s),
                   "H2D im"))
      return;
  }
  {
    OpTimer t(c, TNS_OP_COL2IM);
    if (hip_status(launch_col2im(g, dCol, colElems, dIm, imgElems, batchCount, s), "col2im"))
      return;
  }
  for (int64_t b = 0; b < batchCount; ++b)
    if (hip_status(hipMemcpyAsync(outData + outOffset + b * outStride, dIm + b * imgElems,
                                  imgElems * 4, hipMemcpyDeviceToHost, s),
                   "D2H im"))
      return;
  hip_status(hipStreamSynchronize(s), "sync");
}

void tns_col2im(int64_t aChannels, int64_t aHeight, int64_t aWidth, int64_t kernelHeight,
                int64_t kernelWidth, int64_t padHeight, int64_t padWidth, int64_t strideY,
                int64_t strideX, int64_t dilationY, int64_t dilationX, const float* inData,
                int64_t inOffset, float* outData, int64_t outOffset, int64_t batch,
                uint8_t multiThread) {
  (void)batch;        // scol2im's `batch` argument is unused by the reference too
  (void)multiThread;  // race-free gather; matches the single-threaded order
  tns_col2im_strided_batched(aChannels, aHeight, aWidth, kernelHeight, kernelWidth, padHeight,
                             padWidth, strideY, strideX, dilationY, dilationX, inData, 0,
                             inOffset, outData, 0, outOffset, 1);
}

}  // extern "C"
