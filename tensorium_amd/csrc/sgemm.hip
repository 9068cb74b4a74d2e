// sgemm.hip — SGEMM dispatch: tile-shape choice per problem and the variant
// table used by the tuning entry point (tns_hip_gemm_variant).  The kernel
// itself (MFMA main loop, numerics notes) is in sgemm_kernel.hpp.
#include <cmath>

#include "sgemm_kernel.hpp"

namespace tns {
namespace {

#define TNS_ROW(ID, NAME, BMv, BNv, KIND) &launch_shape_##ID,
const ShapeLauncher kLaunchers[] = {TNS_SHAPES(TNS_ROW)};
#undef TNS_ROW
constexpr int kNumVariants = kNumTileVariants;
static_assert(sizeof(kLaunchers) / sizeof(kLaunchers[0]) == kNumVariants, "one launcher per shape");

unsigned* g_stamps = nullptr;  // block timeline buffer (diagnostic builds only)

// (the tile choice of a plain GEMM: pick_tile_variant, gemm_plan.cpp)

// Implicit-GEMM conv tile choice.  No split-K (bit-exactness), so the
// parallelism is the output tiles alone.  From the YOLOv3 sweep (scripts/
// conv_sweep.py; b64 = blocks a 64x64 tile would give):
//   b64 >= 1200, filters % 128 == 0  128x64, 8 waves of 32x32
//   b64 >= 600 (or 64 filters)       64x64, 8 waves of 32x16 (16x16 MFMA)
//   fewer blocks: 16x16-MFMA tiles, whose four times as many accumulator
//   chains per output area keep 256 CUs busy — 64x32 for deep K (the
//   1024-filter 3x3 layers), 32x32 for the fewest blocks, else 32x64.
int pick_conv_variant(const GemmArgs& a) {
  const int64_t M = a.M, N = a.N, K = a.K;
  if (M <= 32) return V_32x32m16;
  const int64_t b64 = ((M + 63) / 64) * ((N + 63) / 64);
  if (b64 >= 1200 && M % 128 == 0) return V_128x64w8;
  if (b64 >= 600) return V_64x64w8m16;
  if (K >= 2048) return V_64x32m16;
  if (b64 <= 200) return V_32x32m16;
  return V_32x64m16;
}

}  // namespace

hipError_t launch_sgemm_conv_variant(int variant, const GemmArgs& a_in, hipStream_t s) {
  GemmArgs a = a_in;
  a.stamps = g_stamps;
  if (a.M <= 0 || a.N <= 0 || a.batch <= 0) return hipSuccess;
  if (!a.conv || !a.ktab) return hipErrorInvalidValue;
  const bool av = vec4_ok((reinterpret_cast<uintptr_t>(a.A) & 15) == 0, a.lda, a.strideA, a.batch, a.K);
  const int v = variant < 0 ? pick_conv_variant(a) : variant;
  switch (v) {
    case V_128x64: return launch_conv_128x64(a, av, s);
    case V_64x128: return launch_conv_64x128(a, av, s);
    case V_32x256: return launch_conv_32x256(a, av, s);
    case V_64x64: return launch_conv_64x64(a, av, s);
    case V_64x64m16: return launch_conv_64x64m16(a, av, s);
    case V_32x32m16: return launch_conv_32x32m16(a, av, s);
    case V_64x32m16: return launch_conv_64x32m16(a, av, s);
    case V_32x64m16: return launch_conv_32x64m16(a, av, s);
    case V_128x64w8: return launch_conv_128x64w8(a, av, s);
    case V_64x128w8: return launch_conv_64x128w8(a, av, s);
    case V_128x128w8: return launch_conv_128x128w8(a, av, s);
    case V_64x64d1: return launch_conv_64x64d1(a, av, s);
    case V_64x64w8m16: return launch_conv_64x64w8m16(a, av, s);
    default: return hipErrorInvalidValue;  // no implicit-conv instantiation
  }
}

hipError_t launch_sgemm_conv(const GemmArgs& a, hipStream_t s) {
  return launch_sgemm_conv_variant(-1, a, s);
}

// the last variant indices are the dedicated large-NN kernels (sgemm_nn_big.hip)
int sgemm_variant_count() { return kNumVariants + sgemm_nn_big_count(); }
const char* sgemm_variant_name(int v) {
  if (v >= kNumVariants) return sgemm_nn_big_name(v - kNumVariants);
  return (v >= 0 && v < kNumVariants) ? tile_variant(v).name : "";
}

// the executors read the plan and nothing else
hipError_t launch_gemm_plan(const GemmPlan& p, const GemmArgs& a_in, hipStream_t s) {
  if (p.err) return hipErrorInvalidValue;
  switch (p.family) {
    case GEMM_EMPTY: return hipSuccess;
    case GEMM_TILE: {
      GemmArgs a = a_in;
      a.stamps = g_stamps;
      return kLaunchers[p.form](a, p.ta, p.tb, p.vec_a == 4, p.vec_b == 4, s);
    }
    case GEMM_NN_BIG: {
      GemmArgs a = a_in;
      a.stamps = g_stamps;
      return launch_sgemm_nn_big(p, a, s);
    }
    case GEMM_NT_SDOT: return launch_sgemm_nt_sdot_tn(p, a_in, s);
    case GEMM_SDOT_CHAINS: return launch_sdot_chains(a_in, p.form, s);
    case GEMM_SDOT_RC: return launch_sdot_rc(p.form, a_in, s);
    case GEMM_TT: return launch_sgemm_tt_plan(p, a_in, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_sgemm_variant(int variant, const GemmArgs& a, bool transA, bool transB,
                                hipStream_t s) {
  if (variant >= sgemm_variant_count()) return hipErrorInvalidValue;
  return launch_gemm_plan(plan_gemm_variant(gemm_shape(a, transA, transB), variant), a, s);
}

hipError_t launch_sgemm(const GemmArgs& a, bool transA, bool transB, hipStream_t s) {
  return launch_sgemm_variant(-1, a, transA, transB, s);
}

#ifdef TNS_GEMM_STAMPS
// diagnostic build only (not in include/tns.h): every following launch
// records {start, end, HW_ID, XCC_ID} per block into dev_buf (8 words per
// block), or nothing when dev_buf is NULL
extern "C" int tns_debug_gemm_stamps(unsigned* dev_buf) {
  g_stamps = dev_buf;
  return 0;
}
#endif

}  // namespace tns
