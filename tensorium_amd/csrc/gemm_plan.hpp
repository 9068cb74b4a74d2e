// gemm_plan.hpp — which kernel an SGEMM runs on, decided by pure host
// functions of the problem's shape and the options: no context, no HIP call,
// no allocation, no global.  The launchers (sgemm.hip, sgemm_nn_big.hip,
// sgemm_nn_w4.hip, sgemm_nn_pp.hip, sgemm_sdot.hip, sgemm_tt.hip, do_gemm in
// tns_ctx.hpp) read the plan these give and hold no rule of their own; what
// only a launch knows (a grid past the hardware's limit) stays with them.
#pragma once
#include <stdint.h>

namespace tns {

// the tile shapes of sgemm_kernel.hpp's template, in tuning-table order.
// KIND: launch_full  every transpose x A, B staged by float4 or by element
//       launch_trans4  every transpose, both operands float4 only
//       launch_nn4     NN with both operands float4 only
#define TNS_SHAPES(X)                                    \
  X(128x128, "128x128x32_w2x2", 128, 128, launch_full)   \
  X(128x64, "128x64x32_w2x2", 128, 64, launch_full)      \
  X(64x128, "64x128x32_w2x2", 64, 128, launch_full)      \
  X(64x256, "64x256x32_w1x4", 64, 256, launch_full)      \
  X(32x256, "32x256x32_w1x4", 32, 256, launch_full)      \
  X(256x256w8, "256x256x32_w2x4", 256, 256, launch_trans4) \
  X(64x64, "64x64x32_w2x2", 64, 64, launch_full)          \
  X(256x256, "256x256x32_w2x2", 256, 256, launch_nn4)    \
  X(256x256k16, "256x256x16_w2x2", 256, 256, launch_nn4) \
  X(256x128, "256x128x32_w2x2", 256, 128, launch_nn4)    \
  X(128x256, "128x256x32_w2x2", 128, 256, launch_nn4)    \
  X(256x128k16, "256x128x16_w2x2", 256, 128, launch_nn4) \
  X(64x64m16, "64x64x32_w2x2_m16", 64, 64, launch_full)  \
  X(32x32m16, "32x32x32_w2x2_m16", 32, 32, launch_full)  \
  X(64x32m16, "64x32x32_w2x2_m16", 64, 32, launch_nn4)   \
  X(32x64m16, "32x64x32_w2x2_m16", 32, 64, launch_nn4)   \
  X(128x128m16, "128x128x32_w2x2_m16", 128, 128, launch_nn4) \
  X(256x256w8m16, "256x256x32_w2x4_m16", 256, 256, launch_trans4) \
  X(128x64w8, "128x64x32_w4x2", 128, 64, launch_nn4)     \
  X(64x128w8, "64x128x32_w2x4", 64, 128, launch_nn4)     \
  X(128x128w8, "128x128x32_w4x2", 128, 128, launch_nn4)  \
  X(64x64d1, "64x64x32_w2x2_d1", 64, 64, launch_nn4)     \
  X(64x64w8m16, "64x64x32_w2x4_m16", 64, 64, launch_nn4)

enum TileKind { KIND_launch_full = 0, KIND_launch_trans4 = 1, KIND_launch_nn4 = 2 };
enum {
#define TNS_ENUM(ID, NAME, BMv, BNv, KIND) V_##ID,
  TNS_SHAPES(TNS_ENUM)
#undef TNS_ENUM
  kNumTileVariants
};
struct TileVariant {
  const char* name;
  int bm, bn, kind;
};
const TileVariant& tile_variant(int v);  // v in [0, kNumTileVariants)

// what a tile KIND instantiates: launch_trans4 and launch_nn4 return
// hipErrorInvalidValue exactly where this is false
constexpr bool tile_kind_supports(int kind, bool ta, bool tb, bool av, bool bv) {
  return kind == KIND_launch_full ? true
         : kind == KIND_launch_trans4 ? (av && bv)
                                      : (!ta && !tb && av && bv);
}

// float4 staging needs 16-B aligned rows and a contiguous extent that is a
// multiple of 4 (so every float4 is wholly inside or outside the operand)
constexpr bool vec4_ok(bool aligned16, int64_t ld, int64_t stride, int64_t batch, int64_t extent) {
  return aligned16 && ld % 4 == 0 && extent % 4 == 0 && !(batch > 1 && stride % 4 != 0);
}

// the dedicated large-NN kernels' tiles (sgemm_nn_big.hip forms 0..4, the
// ping-pong form 5 of sgemm_nn_pp.hip, forms 6..8 of sgemm_nn_w4.hip)
struct NnBigGeo {
  int bm, bn, bk;
  bool off32;  // addresses A rows and a block's C rows by 32-bit byte offsets
};
constexpr int kNnBigForms = 9;
constexpr NnBigGeo kNnBigGeo[kNnBigForms] = {
    {256, 256, 32, false}, {128, 128, 32, false}, {256, 128, 32, false},
    {256, 256, 32, false}, {256, 128, 16, false}, {256, 256, 32, false},
    {256, 256, 32, true},  {256, 256, 32, true},  {256, 256, 32, true}};
// sgemm_nn_w4.hip: the rows schedule's two ends are two k-tiles each; the
// picked (rows) form holds its loop's fragment addresses in registers from
// kW4PreMinTiles k-tiles on (measured slower below: K = 128, no regular tile,
// by 0.5 us; level from 160 to 384, faster from 512)
constexpr int kW4RowsMinTiles = 4, kW4PreMinTiles = 8;

// sgemm_sdot_rc.hip's k-tile (its buffer offsets run this far past an image)
constexpr int kSdotRcBk = 64;
// TNS_OPT_SDOT_FORM: -1 heuristic, 0 the MFMA kernel, 1 + v chains variant v,
// 64 + v residue-register form v
constexpr int SDOT_FORM_RC = 64;

// a GEMM as the planner sees it: GemmArgs without the pointers
struct GemmShape {
  bool ta = false, tb = false;
  int64_t M = 0, N = 0, K = 0, lda = 0, ldb = 0, ldc = 0;
  int64_t strideA = 0, strideB = 0, strideC = 0, batch = 1;
  bool alpha1 = true;  // alpha == 1
  int beta_mode = 0;   // BetaMode
  int epi = 0;         // EpiKind
  bool conv = false;   // an implicit-GEMM convolution (never a large-NN form)
  bool a16 = true, b16 = true;  // A / B 16-byte aligned
};

enum GemmFamily {
  GEMM_EMPTY = 0,    // no output element: nothing runs
  GEMM_TILE,         // sgemm_kernel.hpp tile `form` of the tuning table
  GEMM_NN_BIG,       // sgemm_nn_big.hip / _pp / _w4 form `form`
  GEMM_NT_SDOT,      // sgemm_sdot.hip launch_tn<tn, vec, bk, o32>
  GEMM_SDOT_CHAINS,  // sgemm_sdot_chains.hip variant `form`
  GEMM_SDOT_RC,      // sgemm_sdot_rc.hip form `form`
  GEMM_TT,           // sgemm_tt.hip, `tn` x `tn` outputs a thread
  GEMM_FAMILIES
};
const char* gemm_family_name(int family);

struct GemmPlan {
  int err = 0;  // TNS_ERR_UNSUPPORTED and its message where a forced form refuses
  char msg[160] = {};
  int family = GEMM_EMPTY;
  int form = -1;  // index in the family's table (GEMM_NT_SDOT: its leaf, 0..6)
  const char* name = "";
  int leaf = -1;  // index of gemm_plan_leaf_name: the kernel instantiation
  bool ta = false, tb = false;  // GEMM_TILE: the transposes it is instantiated for
  // GEMM_TILE: staging widths (4 or 1) of A and B; GEMM_SDOT_CHAINS: both 4
  // (float4 global loads) or both 1
  int vec_a = 0, vec_b = 0;
  // GEMM_NN_BIG forms 6..8: the w4 kernel's template arguments
  bool rows = false, pre = false, alpha1 = false;
  // GEMM_NT_SDOT: launch_tn<tn, vec, bk, o32>; GEMM_TT: tn = outputs a thread
  int tn = 0, vec = 0, bk = 0;
  bool o32 = false;
};

struct Options;  // tns_ctx.hpp

// the pickers, each the one copy of its rule
int pick_tile_variant(const GemmShape& s, bool av, bool bv);
bool nn_big_applies(int form, const GemmShape& s);
int nn_big_pick(const GemmShape& s);  // -1 where none applies by heuristic
bool sdot_rc_applies(const GemmShape& s);

// variant < 0: by shape; else tile `variant` of the table, or large-NN form
// variant - kNumTileVariants (launch_sgemm_variant)
GemmPlan plan_gemm_variant(const GemmShape& s, int variant);
// gemm(NoTrans, Trans) in the sdot order (launch_sgemm_nt_sdot); sdot_form as
// TNS_OPT_SDOT_FORM
GemmPlan plan_gemm_nt_sdot(const GemmShape& s, int sdot_form);
GemmPlan plan_gemm_tt(const GemmShape& s);  // launch_sgemm_tt
// do_gemm: routes by transpose, epilogue and the options nt_sdot / tt_exact
GemmPlan plan_gemm(const GemmShape& s, int variant, const Options& o, int sdot_form);

// every kernel instantiation a plan can name
int gemm_plan_leaf_count();
const char* gemm_plan_leaf_name(int leaf);

}  // namespace tns
