// gemm_plan.cpp — the SGEMM dispatch as pure functions (gemm_plan.hpp) and
// their C entry point, tns_gemm_plan.
#include "gemm_plan.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tns_ctx.hpp"

namespace tns {
namespace {

#define TNS_ROW(ID, NAME, BMv, BNv, KIND) {NAME, BMv, BNv, KIND_##KIND},
const TileVariant kTiles[] = {TNS_SHAPES(TNS_ROW)};
#undef TNS_ROW
static_assert(sizeof(kTiles) / sizeof(kTiles[0]) == kNumTileVariants, "one row per shape");

const char* kTrans[] = {"nn", "nt", "tn", "tt"};
const char* kNtSdotNames[] = {"tn<2,4,64>", "tn<2,1,64,o32>", "tn<2,1,64>", "tn<1,4,256>",
                              "tn<1,1,256>", "tn<1,4,64>",    "tn<1,1,64>"};
constexpr int kNtSdotLeaves = 7;

// leaf order: tiles (each KIND's instantiations), large-NN forms 0..5, the w4
// kernel's <alpha1, rows, pre>, launch_tn's, chains variants x global-load
// width, residue-register forms, the two tt tiles
struct Leaves {
  std::vector<std::string> names;
  int tile0[kNumTileVariants];
  int big0, w40, nt0, chains0, rc0, tt0;
  Leaves() {
    for (int v = 0; v < kNumTileVariants; ++v) {
      tile0[v] = (int)names.size();
      for (int t = 0; t < 4; ++t)
        for (int w = 0; w < 4; ++w) {
          const bool av = !(w & 2), bv = !(w & 1);
          if (!tile_kind_supports(kTiles[v].kind, t & 2, t & 1, av, bv)) continue;
          names.push_back(std::string("tile/") + kTiles[v].name + "/" + kTrans[t] + "/a" +
                          (av ? "4" : "1") + "b" + (bv ? "4" : "1"));
        }
    }
    big0 = (int)names.size();
    for (int f = 0; f < 6; ++f) names.push_back(std::string("nn_big/") + sgemm_nn_big_name(f));
    w40 = (int)names.size();
    for (int i = 0; i < 8; ++i)
      names.push_back(std::string("nn_big/w4<alpha1=") + (i & 4 ? "1" : "0") + ",rows=" +
                      (i & 2 ? "1" : "0") + ",pre=" + (i & 1 ? "1" : "0") + ">");
    nt0 = (int)names.size();
    for (int i = 0; i < kNtSdotLeaves; ++i) names.push_back(std::string("nt_sdot/") + kNtSdotNames[i]);
    chains0 = (int)names.size();
    for (int v = 0; v < sdot_chains_variant_count(); ++v)
      for (int gl = 0; gl < 2; ++gl)
        names.push_back(std::string("sdot_chains/") + sdot_chains_variant_name(v) +
                        (gl ? "/v4" : "/v1"));
    rc0 = (int)names.size();
    for (int v = 0; v < sdot_rc_variant_count(); ++v)
      names.push_back(std::string("sdot_rc/") + sdot_rc_variant_name(v));
    tt0 = (int)names.size();
    names.push_back("tt/r4");
    names.push_back("tt/r8");
  }
  // the tile leaf of (v, ta, tb, av, bv): its rank among the KIND's instantiations
  int tile(int v, bool ta, bool tb, bool av, bool bv) const {
    int n = tile0[v];
    for (int t = 0; t < 4; ++t)
      for (int w = 0; w < 4; ++w) {
        const bool a = !(w & 2), b = !(w & 1);
        if (!tile_kind_supports(kTiles[v].kind, t & 2, t & 1, a, b)) continue;
        if ((bool)(t & 2) == ta && (bool)(t & 1) == tb && a == av && b == bv) return n;
        ++n;
      }
    return -1;
  }
};
const Leaves& leaves() {
  static const Leaves l;
  return l;
}

GemmPlan refuse(GemmPlan p, const char* fmt, ...) {
  p.err = TNS_ERR_UNSUPPORTED;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(p.msg, sizeof(p.msg), fmt, ap);
  va_end(ap);
  return p;
}

bool empty(const GemmShape& s) { return s.M <= 0 || s.N <= 0 || s.batch <= 0; }

GemmPlan plan_tile(const GemmShape& s, int v, bool av, bool bv) {
  GemmPlan p;
  p.family = GEMM_TILE;
  p.form = v;
  p.name = kTiles[v].name;
  p.ta = s.ta;
  p.tb = s.tb;
  p.vec_a = av ? 4 : 1;
  p.vec_b = bv ? 4 : 1;
  if (!tile_kind_supports(kTiles[v].kind, s.ta, s.tb, av, bv))
    return refuse(p, "tile %s is %s", p.name,
                  kTiles[v].kind == KIND_launch_nn4 ? "NN with float4 operands only"
                                                    : "float4 operands only");
  p.leaf = leaves().tile(v, s.ta, s.tb, av, bv);
  return p;
}

GemmPlan plan_nn_big(const GemmShape& s, int form) {
  GemmPlan p;
  p.family = GEMM_NN_BIG;
  p.form = form;
  p.name = sgemm_nn_big_name(form);
  if (form < 0 || form >= kNnBigForms) return refuse(p, "no large-NN form %d", form);
  if (s.ta || s.tb) return refuse(p, "large-NN form %s: NN only", p.name);
  if (!nn_big_applies(form, s))
    return refuse(p, "large-NN form %s: M, N, K multiples of %d, %d, %d, 16-byte aligned rows, "
                  "plain epilogue", p.name, kNnBigGeo[form].bm, kNnBigGeo[form].bn,
                  kNnBigGeo[form].bk);
  if (form < 6) {
    p.leaf = leaves().big0 + form;
    return p;
  }
  // forms 6 (rows, pre), 7 (flat, pre), 8 (rows, no pre), each where K has the tiles
  const bool rows_asked = form != 7, pre_asked = form != 8;
  const int64_t nt = s.K / kNnBigGeo[form].bk;
  p.pre = pre_asked && (!rows_asked || nt >= kW4PreMinTiles);
  p.rows = rows_asked && nt >= kW4RowsMinTiles;
  p.alpha1 = s.alpha1;
  p.leaf = leaves().w40 + (p.alpha1 ? 4 : 0) + (p.rows ? 2 : 0) + (p.pre ? 1 : 0);
  return p;
}

GemmPlan plan_tn(int i, int tn, int vec, int bk, bool o32) {
  GemmPlan p;
  p.family = GEMM_NT_SDOT;
  p.form = i;
  p.name = kNtSdotNames[i];
  p.leaf = leaves().nt0 + i;
  p.tn = tn; p.vec = vec; p.bk = bk; p.o32 = o32;
  return p;
}

GemmPlan plan_chains(const GemmShape& s, int v) {
  GemmPlan p;
  p.family = GEMM_SDOT_CHAINS;
  p.form = v;
  p.name = sdot_chains_variant_name(v);
  if (v < 0 || v >= sdot_chains_variant_count()) return refuse(p, "no chains variant %d", v);
  const bool gl = vec4_ok(s.a16, s.lda, s.strideA, s.batch, s.K) &&
                  vec4_ok(s.b16, s.ldb, s.strideB, s.batch, s.K);
  p.vec_a = p.vec_b = gl ? 4 : 1;
  p.leaf = leaves().chains0 + 2 * v + (gl ? 1 : 0);
  return p;
}

GemmPlan plan_rc(const GemmShape& s, int v) {
  GemmPlan p;
  p.family = GEMM_SDOT_RC;
  p.form = v;
  p.name = sdot_rc_variant_name(v);
  if (v < 0 || v >= sdot_rc_variant_count()) return refuse(p, "no residue-register form %d", v);
  if (!sdot_rc_applies(s))
    return refuse(p, "residue-register form %s: an image's operands past 31-bit byte offsets",
                  p.name);
  p.leaf = leaves().rc0 + v;
  return p;
}

}  // namespace

const TileVariant& tile_variant(int v) { return kTiles[v]; }

const char* gemm_family_name(int f) {
  static const char* n[] = {"empty", "tile", "nn_big", "nt_sdot", "sdot_chains", "sdot_rc", "tt"};
  return f >= 0 && f < GEMM_FAMILIES ? n[f] : "";
}

int gemm_plan_leaf_count() { return (int)leaves().names.size(); }
const char* gemm_plan_leaf_name(int l) {
  return l >= 0 && l < gemm_plan_leaf_count() ? leaves().names[l].c_str() : "";
}

// Shape heuristic: skinny-M conv GEMMs (filters 32/64) get short, wide tiles;
// otherwise the largest tile that still gives every CU work.
// TN with k <= 1024 (the conv backward's col = W^T . delta, K = filters)
// unless 256x256 tiles cover M x N exactly: 64x64 tiles on 16x16 MFMAs, on
// 32x32 MFMAs at k = 1024, 32x32 tiles below ~2 blocks per CU (scripts/
// sgemm_sweep.py --tn, YOLOv3 dX shapes at batch 8: 52^2 3x3 70 -> 88 TF,
// 26^2 83 -> 92, 13^2 68 -> 72, 1x1 layers 38-52 -> 47-60; 4096^2 x 1024
// stays on 256x256, 121 TF against 106 on 64x64).
//
// NN with float4 operands (the conv GEMMs of Conv2D and forwardGPU's
// gemmStridedBatched, strideA = 0; FC dX) by block count, as the implicit
// conv picks (b64 = blocks a 64x64 tile gives, batch included): skinny M on
// 32x64 / 64x128 tiles, >= 1200 blocks of a deep K on 128x64, >= 600 on
// 8-wave 64x64 16x16-MFMA tiles, fewer on 64x32 / 32x32 16x16-MFMA tiles
// (profiles/r03_sgemm_sweep_yolo.json: every YOLOv3 batch-8 shape within
// 10 % of the best swept tile; the old N >= 1024 rule was up to 2.4x off).
int pick_tile_variant(const GemmShape& a, bool av, bool bv) {
  const bool ta = a.ta, tb = a.tb;
  const int64_t M = a.M, N = a.N, batch = a.batch;
  auto blocks = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn) * batch; };
  const bool big_exact = M % 256 == 0 && N % 256 == 0 && blocks(256, 256) >= 240 && av && bv;
  if (ta && !tb && a.K <= 1024 && M > 64 && !big_exact)
    return blocks(64, 64) < 512 ? V_32x32m16 : (a.K >= 1024 ? V_64x64 : V_64x64m16);
  if (!ta && !tb && !big_exact) {
    // the 8-wave and 64x32 / 32x64 shapes are float4-NN only: their
    // nearest general shape otherwise (N = 169 etc. is not a multiple of 4)
    const bool v4 = av && bv;
    const int64_t b64 = blocks(64, 64);
    if (M <= 32) {
      if (a.K < 32) return V_32x256;
      return blocks(32, 64) >= 1024 && v4 ? V_32x64m16 : V_32x32m16;
    }
    if (M <= 64) return b64 >= 600 ? (v4 ? V_64x128w8 : V_64x128) : V_32x32m16;
    if (b64 >= 1200 && M % 128 == 0 && a.K >= 1024) return V_128x64;
    if (b64 >= 600) return v4 ? V_64x64w8m16 : V_64x64;
    if (b64 >= 256 && a.K < 2048 && v4) return V_64x32m16;
    return V_32x32m16;
  }
  if (M <= 32) return V_32x256;
  if (M <= 64) return V_64x256;
  if (M >= 256 && blocks(256, 256) >= 240 && av && bv) return V_256x256w8;
  if (N >= 1024) return V_64x128;
  return V_128x64;
}

bool nn_big_applies(int form, const GemmShape& a) {
  if (form < 0 || form >= kNnBigForms) return false;
  const NnBigGeo& g = kNnBigGeo[form];
  if (a.ta || a.tb || a.conv || a.epi != EPI_NONE || a.beta_mode == BETA_STORE) return false;
  if (a.M % g.bm || a.N % g.bn || a.K % g.bk || a.M <= 0 || a.N <= 0) return false;
  if (a.lda % 4 || a.ldb % 4 || !a.a16 || !a.b16) return false;
  if (a.batch > 1 && (a.strideA % 4 || a.strideB % 4)) return false;
  // (32-bit byte offsets: 7 rows of A per DMA lane offset, a block's 256
  // rows of C from its first row)
  if (g.off32 && (a.lda * 4 * 8 > 0x7fffffffLL || (256 * a.ldc + a.N) * 4 > 0x7fffffffLL))
    return false;
  return (a.M / g.bm) * (a.N / g.bn) <= 0x7fffffff;
}

// heuristic: the 256x256 tile when it gives about a block per CU, at one
// wave per SIMD with LDS-DMA operands where it applies (form 6; 4096^3 0.983
// -> 0.950 ms against the ping-pong form 5, which itself took 0.994 -> 0.972
// from form 0; all bit-identical).  Form 6 runs its row-ordered schedule
// wherever K >= 128 and the flat one (form 7) below: rows measured faster
// than flat by more than flat's round-to-round spread at every K (128 ..
// 4096) and beta mode tried (4096^3 0.9545 -> 0.9393 ms, 1024 x 1024^3 16.37
// -> 16.09; profiles/sgemm_w4_rows_ab.json), so no shape picks form 7.  From
// K = 256 on form 6 holds its loop's fragment addresses in registers (4096^3
// 0.9364 -> 0.9167 ms against form 8, which computes them per step; K = 128
// measured slower that way and 160 .. 384 level, so below 256 form 6 is form
// 8's kernel; profiles/sgemm_w4_afrag_ab.json)
int nn_big_pick(const GemmShape& a) {
  if (nn_big_applies(0, a) && (a.M / 256) * (a.N / 256) * a.batch >= 192)
    return nn_big_applies(6, a) ? 6 : nn_big_applies(5, a) ? 5 : 0;
  return -1;
}

// every image's operands, and the rows a last tile runs past them,
// byte-addressable in 31 bits (buffer offsets)
bool sdot_rc_applies(const GemmShape& a) {
  const int64_t ea = (a.M + 128) * a.lda + a.K + kSdotRcBk,
                eb = (a.N + 128) * a.ldb + a.K + kSdotRcBk;
  return a.M > 0 && a.N > 0 && a.K >= 0 && a.lda >= a.K && a.ldb >= a.K &&
         ea * 4 < 0x7fffffffLL && eb * 4 < 0x7fffffffLL;
}

GemmPlan plan_gemm_variant(const GemmShape& a, int variant) {
  if (empty(a)) return GemmPlan{};
  // A is k-contiguous unless transposed; B is n-contiguous unless transposed
  const bool av = vec4_ok(a.a16, a.lda, a.strideA, a.batch, a.ta ? a.M : a.K);
  const bool bv = vec4_ok(a.b16, a.ldb, a.strideB, a.batch, a.tb ? a.K : a.N);
  // the last variant indices are the dedicated large-NN kernels
  if (variant >= kNumTileVariants) return plan_nn_big(a, variant - kNumTileVariants);
  if (variant < 0 && !a.ta && !a.tb) {
    const int nb = nn_big_pick(a);
    if (nb >= 0) return plan_nn_big(a, nb);
  }
  return plan_tile(a, variant < 0 ? pick_tile_variant(a, av, bv) : variant, av, bv);
}

// MFMA: 32x64 tiles when they still give >= 4 blocks per CU, else 32x32;
// few outputs over a long k go to the VALU chain kernel
GemmPlan plan_gemm_nt_sdot(const GemmShape& a, int sdot_form) {
  if (empty(a)) return GemmPlan{};
  if (sdot_form >= SDOT_FORM_RC) return plan_rc(a, sdot_form - SDOT_FORM_RC);
  if (sdot_form > 0) return plan_chains(a, sdot_form - 1);
  // few outputs over a long k (conv dW of the 416/208/104-pixel YOLOv3
  // layers): the VALU chain kernel, tile by output count (scripts/
  // sdot_forms.py, profiles/r02_sdot_forms.json: YOLOv3 layer 0 dW at batch
  // 8 1.44 -> 0.28 ms, layer 2 0.35 -> 0.10 ms, layer 5 0.089 -> 0.056 ms;
  // the 104^2 1x1 layers' 65536 outputs on four residues a lane, 0.130 ->
  // 0.115 ms a call, profiles/r04_bwd_dw_sweep.json)
  const int64_t t32 = ((a.M + 31) / 32) * ((a.N + 31) / 32) * a.batch;
  if (sdot_form < 0 && a.K >= 4096 && t32 <= 64) {
    const int64_t outs = a.M * a.N * a.batch;
    return plan_chains(a, outs <= 8192 ? 1 : (outs <= 32768 ? 2 : 6));
  }
  // many 64x64 tiles over a short k (conv dW of the 26^2 / 13^2 layers, k =
  // pixels per image): two waves per 32x32 tile, four residue chains each
  // (sgemm_sdot_rc.hip; profiles/r03_dw_forms.json: 4-7 % on those layers,
  // behind this kernel on the 52^2 ones)
  const int64_t t64 = ((a.M + 63) / 64) * ((a.N + 63) / 64) * a.batch;
  if (sdot_form < 0 && a.K <= 1024 && t64 >= 512 && sdot_rc_applies(a)) return plan_rc(a, 1);
  const bool v = vec4_ok(a.a16, a.lda, a.strideA, a.batch, a.K) &&
                 vec4_ok(a.b16, a.ldb, a.strideB, a.batch, a.K);
  const int64_t b64 = ((a.M + 31) / 32) * ((a.N + 63) / 64) * a.batch;
  // scalar staging with 32-bit row offsets when each image's A and B fit them
  const bool o32 = (a.M - 1) * a.lda + a.K <= 0x7fffffffLL && (a.N - 1) * a.ldb + a.K <= 0x7fffffffLL;
  if (b64 >= 1024)
    return v ? plan_tn(0, 2, 4, 64, false) : (o32 ? plan_tn(1, 2, 1, 64, true) : plan_tn(2, 2, 1, 64, false));
  // few 32x32 tiles over a long k: 256-deep k-tiles (the 64-row LDS stages
  // take 2 x 65.8 KB of gfx950's 160 KB)
  if (a.K >= 16384 && ((a.M + 31) / 32) * ((a.N + 31) / 32) * a.batch < 512)
    return v ? plan_tn(3, 1, 4, 256, false) : plan_tn(4, 1, 1, 256, false);
  return v ? plan_tn(5, 1, 4, 64, false) : plan_tn(6, 1, 1, 64, false);
}

// 128x128 tiles (8x8 per thread) when they still give >= 2 blocks per CU,
// else 64x64 (4x4 per thread)
GemmPlan plan_gemm_tt(const GemmShape& a) {
  if (empty(a)) return GemmPlan{};
  const int64_t b128 = ((a.M + 127) / 128) * ((a.N + 127) / 128) * a.batch;
  GemmPlan p;
  p.family = GEMM_TT;
  p.tn = b128 >= 512 ? 8 : 4;
  p.form = p.tn == 8;
  p.name = p.tn == 8 ? "tt_128x128_r8" : "tt_64x64_r4";
  p.leaf = leaves().tt0 + p.form;
  return p;
}

GemmPlan plan_gemm(const GemmShape& a, int variant, const Options& o, int sdot_form) {
  if (empty(a)) return GemmPlan{};
  if (!a.ta && a.tb && o.nt_sdot && variant < 0 && a.epi == EPI_NONE)
    return plan_gemm_nt_sdot(a, sdot_form);
  if (a.ta && a.tb && o.tt_exact && variant < 0 && a.epi == EPI_NONE) return plan_gemm_tt(a);
  return plan_gemm_variant(a, variant);
}

}  // namespace tns

using namespace tns;

extern "C" {

int tns_gemm_plan_leaf_count(void) { return gemm_plan_leaf_count(); }
const char* tns_gemm_plan_leaf_name(int32_t leaf) { return gemm_plan_leaf_name(leaf); }

int tns_gemm_plan(int32_t variant, const int64_t* in, char* out, int64_t out_len) {
  if (!in || !out || out_len < 1) return set_error(TNS_ERR_ARG, "gemm plan: null argument");
  if (variant >= sgemm_variant_count())
    return set_error(TNS_ERR_ARG, "gemm variant %d out of range", variant);
  GemmShape s;
  s.ta = in[TNS_GP_TRANS_A] != 0;
  s.tb = in[TNS_GP_TRANS_B] != 0;
  s.M = in[TNS_GP_M]; s.N = in[TNS_GP_N]; s.K = in[TNS_GP_K];
  s.lda = in[TNS_GP_LDA]; s.ldb = in[TNS_GP_LDB]; s.ldc = in[TNS_GP_LDC];
  s.strideA = in[TNS_GP_STRIDE_A]; s.strideB = in[TNS_GP_STRIDE_B]; s.strideC = in[TNS_GP_STRIDE_C];
  s.batch = in[TNS_GP_BATCH];
  s.alpha1 = in[TNS_GP_ALPHA_IS_ONE] != 0;
  s.beta_mode = (int)in[TNS_GP_BETA_MODE];
  s.epi = (int)in[TNS_GP_EPI];
  s.a16 = in[TNS_GP_A_ALIGNED16] != 0;
  s.b16 = in[TNS_GP_B_ALIGNED16] != 0;
  if (s.beta_mode < BETA_ZERO || s.beta_mode > BETA_STORE || s.epi < EPI_NONE || s.epi > EPI_ADD)
    return set_error(TNS_ERR_ARG, "gemm plan: bad beta mode or epilogue");
  Options o;  // the defaults, then the three that steer a GEMM
  o.nt_sdot = in[TNS_GP_NT_SDOT];
  o.tt_exact = in[TNS_GP_TT_EXACT];
  const GemmPlan p = plan_gemm(s, variant, o, (int)in[TNS_GP_SDOT_FORM]);
  std::string msg;
  for (const char* c = p.msg; *c; ++c) {
    if (*c == '"' || *c == '\\') msg += '\\';
    msg += *c;
  }
  auto tf = [](bool b) { return b ? "true" : "false"; };
  const int n = snprintf(
      out, (size_t)out_len,
      "{\"err\": %d, \"msg\": \"%s\", \"family\": \"%s\", \"form\": %d, \"name\": \"%s\", "
      "\"leaf\": \"%s\", \"vec_a\": %d, \"vec_b\": %d, \"rows\": %s, \"pre\": %s, \"alpha1\": %s, "
      "\"tn\": %d, \"vec\": %d, \"bk\": %d, \"o32\": %s}",
      p.err, msg.c_str(), gemm_family_name(p.family), p.form, p.name, gemm_plan_leaf_name(p.leaf),
      p.vec_a, p.vec_b, tf(p.rows), tf(p.pre), tf(p.alpha1), p.tn, p.vec, p.bk, tf(p.o32));
  if (n < 0 || n >= out_len) return set_error(TNS_ERR_ARG, "gemm plan: buffer of %lld bytes too small", (long long)out_len);
  return TNS_OK;
}

}  // extern "C"
