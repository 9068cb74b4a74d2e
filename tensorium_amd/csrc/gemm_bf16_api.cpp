// gemm_bf16_api.cpp — the bf16 GEMM entry points of the C ABI (include/tns.h,
// gemm_bf16.hip).  Opt-in reduced precision; no TNNCuda methods, hence no
// tns_hip_ prefix: like tns_conv_bf16_* the entries join the side stream on
// every call (check_ctx) instead of taking a place in the hazard table.
#include "tns_ctx.hpp"

using namespace tns;

namespace {

constexpr int64_t kMaxDim = 0x7fffff00LL;  // 32-bit tile and k indexing

bool meet(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// a rows x cols matrix of leading dimension ld
Span matrix(const float* p, int64_t rows, int64_t cols, int64_t ld) {
  return span(p, (rows - 1) * ld + cols);
}

// the sizes and C of every form; nothing is launched on a refusal
int check_sizes(const char* me, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                int64_t a_cols, const float* C, int64_t ldc) {
  if (M <= 0 || N <= 0 || K <= 0 || M > kMaxDim || N > kMaxDim || K > kMaxDim)
    return set_error(TNS_ERR_ARG, "%s: M %lld, N %lld, K %lld outside [1, 2^31 - 256]", me,
                     (long long)M, (long long)N, (long long)K);
  if (!A || !C) return set_error(TNS_ERR_ARG, "%s: null operand", me);
  if (lda < a_cols || ldc < N)
    return set_error(TNS_ERR_ARG, "%s: leading dimension too small (lda=%lld ldc=%lld)", me,
                     (long long)lda, (long long)ldc);
  return TNS_OK;
}

int run(tns_ctx* c, const char* me, GemmBf16Args& g) {
  const int tile = gemm_bf16_tile(g.M, g_opt.gemm_bf16_tile);
  const int split = (int)gemm_bf16_split(tile, g.M, g.N, g.K, g_opt.gemm_bf16_split,
                                         g_opt.scratch_cap);
  if (split > 1)
    if (int e = ensure_scratch(c, SLOT_BF16_GEMM, split * g.M * g.N, &g.part)) return e;
  OpTimer t(c, TNS_OP_GEMM);
  return hip_status(launch_gemm_bf16(tile, split, g, c->stream), me);
}

}  // namespace

extern "C" {

int tns_gemm_bf16(tns_ctx* c, uint8_t transA, uint8_t transB, int64_t M, int64_t N, int64_t K,
                  const float* A, int64_t lda, const float* B, int64_t ldb, int32_t accumulate,
                  float* C, int64_t ldc) {
  const char* const me = "gemm bf16";
  if (int r = check_ctx(c)) return r;
  if (transA && transB)
    return set_error(TNS_ERR_UNSUPPORTED, "%s: the TT form is not built (NT, TN, NN)", me);
  // row-major: A is M x K (K x M transposed), B is K x N (N x K transposed)
  const int64_t a_rows = transA ? K : M, a_cols = transA ? M : K;
  const int64_t b_rows = transB ? N : K, b_cols = transB ? K : N;
  if (int r = check_sizes(me, M, N, K, A, lda, a_cols, C, ldc)) return r;
  if (!B) return set_error(TNS_ERR_ARG, "%s: null operand", me);
  if (ldb < b_cols)
    return set_error(TNS_ERR_ARG, "%s: leading dimension too small (ldb=%lld)", me,
                     (long long)ldb);
  const Span sc = matrix(C, M, N, ldc);
  if (meet(sc, matrix(A, a_rows, a_cols, lda)) || meet(sc, matrix(B, b_rows, b_cols, ldb)))
    return set_error(TNS_ERR_ARG, "%s: C overlaps A or B", me);
  GemmBf16Args g{};
  g.form = transA ? GEMM_BF16_TN : transB ? GEMM_BF16_NT : GEMM_BF16_NN;
  g.M = M, g.N = N, g.K = K, g.A = A, g.lda = lda, g.B = B, g.ldb = ldb;
  g.accumulate = accumulate != 0, g.C = C, g.ldc = ldc;
  return run(c, me, g);
}

int tns_gemm_bf16_packed_bytes(tns_ctx* c, int64_t N, int64_t K, int64_t* bytes) {
  if (int r = check_ctx(c)) return r;
  if (N <= 0 || K <= 0 || N > kMaxDim || K > kMaxDim || !bytes)
    return set_error(TNS_ERR_ARG, "gemm bf16 packed bytes: N or K outside [1, 2^31 - 256], or "
                                  "null bytes");
  *bytes = gemm_bf16_packed_bytes(N, K);
  return TNS_OK;
}

int tns_gemm_bf16_pack(tns_ctx* c, int64_t N, int64_t K, const float* W, int64_t ldw,
                       void* packed) {
  const char* const me = "gemm bf16 pack";
  if (int r = check_ctx(c)) return r;
  if (N <= 0 || K <= 0 || N > kMaxDim || K > kMaxDim)
    return set_error(TNS_ERR_ARG, "%s: N %lld, K %lld outside [1, 2^31 - 256]", me, (long long)N,
                     (long long)K);
  if (!W || !packed || !aligned16(packed) || ldw < K)
    return set_error(TNS_ERR_ARG,
                     "%s: null operand, packed not 16-byte aligned, or ldw below K", me);
  if (meet(matrix(W, N, K, ldw),
           span(static_cast<const float*>(packed), gemm_bf16_packed_bytes(N, K) / 4)))
    return set_error(TNS_ERR_ARG, "%s: W and packed overlap", me);
  return hip_status(launch_gemm_bf16_pack(N, K, W, ldw, packed, c->stream), me);
}

int tns_gemm_bf16_nt_packed(tns_ctx* c, int64_t M, int64_t N, int64_t K, const float* A,
                            int64_t lda, const void* packed, int32_t accumulate, float* C,
                            int64_t ldc) {
  const char* const me = "gemm bf16 nt packed";
  if (int r = check_ctx(c)) return r;
  if (int r = check_sizes(me, M, N, K, A, lda, K, C, ldc)) return r;
  if (!packed || !aligned16(packed))
    return set_error(TNS_ERR_ARG, "%s: packed null or not 16-byte aligned", me);
  const Span sc = matrix(C, M, N, ldc);
  if (meet(sc, matrix(A, M, K, lda)) ||
      meet(sc, span(static_cast<const float*>(packed), gemm_bf16_packed_bytes(N, K) / 4)))
    return set_error(TNS_ERR_ARG, "%s: C overlaps A or packed", me);
  GemmBf16Args g{};
  g.form = GEMM_BF16_NT_PACKED;
  g.M = M, g.N = N, g.K = K, g.A = A, g.lda = lda, g.B = packed, g.ldb = 0;
  g.accumulate = accumulate != 0, g.C = C, g.ldc = ldc;
  return run(c, me, g);
}

}  // extern "C"
