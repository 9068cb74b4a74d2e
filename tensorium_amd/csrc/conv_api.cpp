// conv_api.cpp — the convolution entry points of the C ABI (include/tns.h):
// TTensor.Conv2D (ntensors.pas:8252-8349) and TConvolutionalLayer.forward /
// backward (nConvolutionLayer.pas:457-569, 590-670, 1022-1153).
//
// Each layer call is planned, then executed: plan_conv_forward /
// plan_conv_backward (pure: shape and options in, plan out) choose the kernel
// family, its form, the scratch and the schedule; one executor per path runs
// the plan on the context.  Nothing below the planners reads an option.
#include <algorithm>
#include <cstdarg>
#include <cstdio>

#include "tns_ctx.hpp"

using namespace tns;

namespace tns {
namespace {
template <class Plan>
Plan& refuse(Plan& p, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(p.msg, sizeof p.msg, fmt, ap);
  va_end(ap);
  p.err = code;
  return p;
}

// buffer offsets are 32-bit: images of img floats per launch such that the B
// extent stays below 2^31 bytes (and N below 2^31)
int64_t images_per_launch(int64_t img, int64_t outImg) {
  return std::max<int64_t>(
      1, std::min<int64_t>(0x7fffffffLL / (4 * img), 0x7fffffffLL / std::max<int64_t>(outImg, 1)));
}

// dw_tile.hip's operands (the planner picks on the shape fields alone)
DwArgs dw_tile_args(const ConvBwdPlan& p, const float* delta, const float* input) {
  const ConvShape& s = p.s;
  DwArgs da{};
  da.delta = delta; da.x = input; da.part = nullptr;
  da.M = (int)p.i_m; da.N = (int)p.i_n; da.HW = (int)p.i_k;
  da.C = (int)s.C; da.H = (int)s.H; da.W = (int)s.W; da.oW = (int)p.g.ow;
  da.stride = (int)s.stride; da.pad = (int)(s.padding * s.dilation); da.dil = (int)s.dilation;
  da.va = p.i_k % 4 == 0 && p.delta_aligned16;
  da.alpha = 1.0f;
  da.strideA = p.i_m * p.i_k; da.strideX = s.C * s.H * s.W; da.strideP = p.i_m * p.i_n;
  da.batch = s.batch;
  return da;
}
}  // namespace

// TConvolutionalLayer.forward's Conv2D, with forwardBias + activate fused into
// the GEMM epilogue (bias_act) or the bare convolution (the batch-norm path,
// whose statistics need the raw output)
ConvFwdPlan plan_conv_forward(const ConvShape& s, int fused, bool bias_act, const Options& o) {
  ConvFwdPlan p;
  const int64_t batch = s.batch, C = s.C, H = s.H, W = s.W, filters = s.filters, kSize = s.kSize,
                stride = s.stride, padding = s.padding, dilation = s.dilation;
  p.s = s;
  p.oh = out_dim(H, padding, kSize, dilation, stride);
  p.ow = out_dim(W, padding, kSize, dilation, stride);
  p.bias_act = bias_act;
  p.conv_variant = o.conv_variant;
  p.srss_quirk = (int)o.srss_quirk;
  // logistic / tanh: bias in the GEMM epilogue (activation 4 = linear there),
  // the transcendental activation in its own pass
  const bool transc = act_transcendental(s.activation);
  p.epi_act = transc ? 4 : s.activation;
  p.act_tail = bias_act && transc;
  if (!fused) {
    p.path = FWD_UNFUSED;
    return p;
  }
  if (fused < TNS_CONV_UNFUSED || fused > TNS_CONV_IMPLICIT)
    return refuse(p, TNS_ERR_ARG, "conv_forward: unknown schedule %d", fused);
  if (const char* m = geom_error(geom(C, H, W, kSize, kSize, padding, padding, stride, stride,
                                      dilation, dilation)))
    return refuse(p, TNS_ERR_ARG, "%s", m);
  const int64_t outImg = p.oh * p.ow, k = C * kSize * kSize, N = batch * outImg;
  if (p.oh <= 0 || p.ow <= 0 || batch <= 0) return p;
  p.needs_col = kSize != 1 || dilation != 1 || stride != 1;
  // TNS_CONV_FUSED: implicit GEMM (batch folded into N: one launch with the
  // tile shapes of pick_conv_variant, measured at or ahead of the per-image
  // GEMM on every YOLOv3 layer, 1x1 ones included)
  // (a padded 1x1/s1 convolution is left to the reference's direct path,
  // which ignores the padding — ntensors.pas:8286)
  const bool direct_ok = p.needs_col || padding == 0;
  // implicit-GEMM limits (32-bit buffer offsets within one image, k-table
  // entries, 16-bit window offsets); the library choice falls back to the
  // im2col schedule past them
  const int64_t Hpad = H + 2 * padding, Wpad = W + 2 * padding;
  const bool fits = !(k > 0x0fffffffLL - KTAB_PAD || C * Hpad * Wpad * 4 > 0x7fffffffLL ||
                      (kSize - 1) * dilation >= 0x8000);
  if (!(direct_ok && (fused == TNS_CONV_IMPLICIT || (fused == TNS_CONV_FUSED && fits)))) {
    p.path = FWD_IM2COL;
    if (p.needs_col) p.col_elems = batch * k * outImg;
    return p;
  }
  // implicit GEMM: batch folded into N, B gathered from zero-padded images
  p.implicit = true;
  const int64_t cvar = o.conv_variant;
  if (cvar >= 200 && cvar < 500)
    return refuse(p, TNS_ERR_UNSUPPORTED,
                  "conv variant %lld: the ping-pong, LDS-DMA-ring and input-patch tile "
                  "families (200..499) were removed",
                  (long long)cvar);
  // short-k first layers (3-channel 3x3): the direct kernel, one HBM pass
  // (TNS_OPT_CONV_VARIANT >= 0 forces a GEMM tile instead)
  if (cvar < 0 && conv_direct_applies(C, kSize, filters)) {
    p.path = FWD_DIRECT;
    return p;
  }
  // 1x1 / stride-1 layers straight from the input planes (conv1x1.hip)
  // where picked, or forced by TNS_OPT_CONV_VARIANT = 600 + v
  if (kSize == 1 && stride == 1 && padding == 0 && dilation == 1) {
    const int cv = cvar >= 600 ? (int)(cvar - 600)
                   : cvar < 0  ? conv1x1_pick(filters, N, k, outImg)
                               : -1;
    if (cv >= 0) {
      p.path = FWD_CONV1X1;
      p.form = cv;
      return p;
    }
  } else if (cvar >= 600) {
    return refuse(p, TNS_ERR_UNSUPPORTED, "conv1x1 forms need a 1x1 stride-1 unpadded layer");
  }
  // the two-pass slab form (conv_slab.hip) where picked, or forced by
  // TNS_OPT_CONV_VARIANT = 500 + v
  const int sv = cvar >= 500 && cvar < 600    ? (int)(cvar - 500)
                 : cvar < 0 && dilation == 1 ? conv_slab_pick(filters, N, k, kSize)
                                              : -1;
  if (sv >= 0) {
    p.col_elems = conv_slab_floats(sv, N, k);
    if (p.col_elems < 0) return refuse(p, TNS_ERR_ARG, "no conv slab form %d", sv);
    p.path = FWD_SLAB;
    p.form = sv;
    return p;
  }
  // plane-sized tiles with a bounds-checked gather from the unpadded images
  // (conv_tile.hip) where picked, or forced by TNS_OPT_CONV_VARIANT = 100 + v
  // (0..99: the sgemm_kernel.hpp shapes, below)
  const int64_t img0 = C * H * W;
  if ((kSize == 1 || kSize == 3) && k % 32 == 0 && img0 * 4 <= 0x7fffffffLL) {
    int tv = -1;
    if (cvar >= 100) {
      tv = (int)(cvar - 100);
    } else if (cvar < 0) {
      GemmArgs probe{};
      probe.M = filters; probe.N = N; probe.K = k;
      probe.conv_sY = (int)stride;
      // (the pick looks at the weights' alignment only)
      probe.A = reinterpret_cast<const float*>(uintptr_t(s.weights_aligned16 ? 16 : 4));
      probe.lda = k;
      tv = conv_tile_pick(probe, (int)kSize);
    }
    if (tv >= 0) {
      p.path = FWD_TILE;
      p.form = tv;
      p.chunk = images_per_launch(img0, outImg);
      return p;
    }
  }
  // Materialise the zero border (padded images, no bounds checks in the
  // GEMM) when that copy costs under ~5% of the GEMM: copy time
  // ~bytes/4 TB/s vs GEMM ~flops/80 TF/s.
  const double flops = 2.0 * (double)filters * (double)N * (double)k;
  p.padded = padding == 0 ||
             (o.conv_pad < 0 ? 8.0 * (double)(batch * C * Hpad * Wpad) * 400.0 < flops
                             : o.conv_pad == 1);
  const int64_t img = p.padded ? C * Hpad * Wpad : img0;
  // (k-table: 8-byte entries in one buffer resource, window offsets packed
  // in 16 bits)
  if (k > 0x0fffffffLL - KTAB_PAD || img * 4 > 0x7fffffffLL || (kSize - 1) * dilation >= 0x8000)
    return refuse(p, TNS_ERR_ARG, "conv_forward: image too large for the implicit GEMM");
  p.path = FWD_IMPLICIT;
  // (99: the sgemm_kernel.hpp shape heuristic, bypassing conv_tile)
  p.form = cvar == 99 ? -1 : (int)cvar;
  if (p.padded && padding > 0) p.stage1_elems = batch * img;
  p.chunk = images_per_launch(img, outImg);
  return p;
}

ConvBwdPlan plan_conv_backward(const ConvShape& s, bool has_bn, bool has_state_delta,
                               bool delta_aligned16, const Options& o) {
  ConvBwdPlan p;
  const int64_t batch = s.batch, C = s.C, H = s.H, W = s.W, filters = s.filters, kSize = s.kSize,
                stride = s.stride, padding = s.padding, dilation = s.dilation;
  p.s = s;
  p.has_bn = has_bn; p.has_state_delta = has_state_delta; p.delta_aligned16 = delta_aligned16;
  p.srss_quirk = (int)o.srss_quirk;
  p.sched = o.bwd_overlap == 2 ? BWD_PIPELINED : o.bwd_overlap ? BWD_JOINED : BWD_SEQUENTIAL;
  // delta / output are [batch][filters][outH*outW] with the layer's outH =
  // (h + 2p - k) div s + 1 (nConvolutionLayer.pas:92-100); the backward
  // im2col / col2im pad with padding*dilation (640, 665), which yields those
  // columns for the "same" paddings at any dilation — other geometries make
  // the reference read past its workspace and are refused
  const ConvGeom g = p.g = geom(C, H, W, kSize, kSize, padding * dilation, padding * dilation,
                                stride, stride, dilation, dilation);
  if (const char* m = geom_error(g)) return refuse(p, TNS_ERR_ARG, "%s", m);
  const int64_t lh = (H + 2 * padding - kSize) / stride + 1;
  const int64_t lw = (W + 2 * padding - kSize) / stride + 1;
  if (g.oh != lh || g.ow != lw)
    return refuse(p, TNS_ERR_UNSUPPORTED,
                  "conv_backward: dilation %lld with padding %lld gives %lldx%lld im2col "
                  "columns but the layer's output is %lldx%lld (nConvolutionLayer.pas:92-100, "
                  "640)",
                  (long long)dilation, (long long)padding, (long long)g.oh, (long long)g.ow,
                  (long long)lh, (long long)lw);
  const int64_t i_m = p.i_m = filters, i_n = p.i_n = kSize * kSize * C, i_k = p.i_k = g.oh * g.ow;
  p.colSize = i_n * i_k;
  if (batch <= 0 || i_k <= 0 || filters <= 0) return p;
  p.empty = false;
  p.bn_elems = 3 * batch * filters;
  // batchNormBack's five passes as one chain pass over delta, output, x_norm
  // and x (the three reductions) + normalizeDelta deriving and scaling each
  // term as it loads it, where the chain kernels apply
  p.bn_fused = has_bn && o.bn_fused;
  p.derive_sums = !has_bn && o.derive_sums;
  // state.input.im2Col(...) — a 1x1/s1/p0 col matrix is the input itself
  const bool needs_col = p.needs_col = kSize != 1 || stride != 1 || padding != 0 || dilation != 1;
  // state.delta of a 1x1 / stride-1 layer as a 1x1 convolution of the delta
  // planes with W^T on conv1x1.hip, the col2im add in its epilogue (the same
  // chains and the same add as the TN product with EPI_ADD)
  const int dx1 = has_state_delta && o.dx_c1 && o.dx_fused != 2 && !needs_col
                      ? conv1x1_pick(C, batch * i_k, filters, i_k)
                      : -1;
  // state.delta of stride-1 layers without the col matrix (conv_dx.hip)
  const bool fused_dx =
      dx1 < 0 && has_state_delta && dilation == 1 &&
      ((o.dx_fused == 1 && conv_dx_fused_applies(C, H, W, kSize, stride, filters, g.oh, g.ow)) ||
       (o.dx_fused == 2 && conv_dx_fused_fits(C, H, W, stride, filters, g.oh, g.ow)));
  // dW with the im2col matrix generated inside the sdot-order product
  // (dw_tile.hip): no col matrix, no im2col pass
  int dwv = -1;
  if (o.nt_sdot && o.dw_tile != -2 && (kSize == 1 || kSize == 3) && C * H * W < (1LL << 27) &&
      i_n <= 0x7fffffffLL && i_k <= 0x7fffffffLL && batch <= 65535)
    dwv = o.dw_tile >= 0 ? (int)o.dw_tile
                         : dw_tile_pick(dw_tile_args(p, nullptr, nullptr), (int)kSize);
  // without a residue form: the tile, else im2col + one strided-batched sdot
  // launch (each image's sums stored as they are) added to weight_updates
  // image by image, else one NT GEMM per image
  ConvDwChoice& fb = p.dw_fallback;
  fb.path = dwv >= 0 ? DW_TILE : o.nt_sdot && batch > 1 ? DW_SDOT : DW_GEMM;
  fb.form = dwv;
  fb.col = needs_col && dwv < 0;
  fb.part_elems = fb.path == DW_GEMM ? 0 : batch * i_m * i_n;
  p.dw = fb;
  // dW as residue chains in sequence over residue-major copies of delta and
  // the im2col matrix (dw_res.hip): the 3x3 layers with large outputs
  int dwr = -1;
  if (o.nt_sdot && o.dw_res != -2 && o.dw_tile < 0 && batch <= 65535 && i_k >= 64) {
    if (o.dw_res >= 0)
      dwr = (int)o.dw_res;
    else if (kSize == 3)  // (1x1 layers: behind the sdot kernels, 0.048 -> 0.058 ms at 52^2)
      dwr = dw_res_pick(i_m, i_n, i_k, batch);
  }
  // its scratch (residue-major copies, group planes) comes in addition to
  // the caller's workspace
  if (dwr >= 0) {
    const int64_t rowlen = 8 * dw_res_k4(i_k);
    // (a form that folds the images itself has no group planes: one float)
    p.dw = ConvDwChoice{DW_RES, dwr, false,
                        std::max<int64_t>(1, batch * dw_res_groups(dwr) * i_m * i_n)};
    p.dw_res_forced = o.dw_res >= 0;
    p.res_a_elems = batch * i_m * rowlen + 32;
    p.res_b_elems = batch * dw_res_b_rows(dwr, i_n) * rowlen + 32;
  }
  if (has_state_delta) {
    // a 1x1/s1/p0 layer's col2im adds each col element to its own pixel once:
    // the dX product adds into state.delta in its epilogue instead (EPI_ADD,
    // the same add), no col matrix
    p.dx_direct = !needs_col && !fused_dx;
    // state.delta of a stride-1 3x3 layer as one implicit transposed
    // convolution (conv_tile4 DX forms: each tap's filter chain added to the
    // pixel in scol2im's order), no col matrix
    // (stride 2: four such convolutions, one per output pixel parity class,
    // each over the taps col2im adds to that class)
    int dxc = -1;
    if (!fused_dx && kSize == 3 && (stride == 1 || stride == 2) && dilation == 1 &&
        o.dx_conv != -2)
      dxc = o.dx_conv >= 0 ? (int)o.dx_conv
            : stride == 2  ? conv_tile4_dx3s2_pick(batch, C, H, W, filters, kSize, padding)
                           : conv_tile4_dx3_pick(batch, C, H, W, filters, kSize, padding);
    p.dx_col = !fused_dx && !p.dx_direct && dxc < 0;
    if (fused_dx) {
      p.dx = DX_FUSED;
    } else if (dxc >= 0) {
      p.dx = stride == 2 ? DX_CONV3S2 : DX_CONV3;
      p.dx_form = dxc;
    } else {
      // col_b = W^T . delta_b for all images in one launch on conv_tile4's
      // k-major-A forms where they apply, else the TN GEMM
      if (o.dx_tile != -2)
        p.dx_tile = o.dx_tile >= 0 ? (int)o.dx_tile
                                   : conv_tile4_dx_pick(i_n, batch * i_k, i_m, kSize);
      p.dx_tile_forced = o.dx_tile >= 0;
      p.dx = dx1 >= 0 ? DX_CONV1X1 : p.dx_tile >= 0 ? DX_TILE : DX_TN;
      p.dx_form = dx1 >= 0 ? dx1 : p.dx_tile;
    }
    if (fused_dx || dxc >= 0 || dx1 >= 0) p.wt_elems = filters * C * kSize * kSize;
  }
  if (p.dw.col || fb.col || p.dx_col) p.col_elems = batch * p.colSize;
  return p;
}

}  // namespace tns

// ---- forward -------------------------------------------------------------------
int tns_hip_conv2d(tns_ctx* c, int64_t batch, int64_t C, int64_t H, int64_t W,
                   const float* input, const float* weights, int64_t filters, int64_t kH,
                   int64_t kW, int64_t wPadding, int64_t hPadding, int64_t xStride,
                   int64_t yStride, int64_t xDilation, int64_t yDilation, float* workspace,
                   float* out) {
  if (int r = check_ctx(c)) return r;
  // ntensors.pas:8266-8269: negative padding => "same"-style default
  if (wPadding < 0) wPadding = xDilation + kW / 2 - 1;
  if (hPadding < 0) hPadding = yDilation + kH / 2 - 1;
  // Conv2D hands (xDilation, yDilation) to im2col's (dilationY, dilationX)
  // slots (ntensors.pas:8303); keep the swap so non-square dilation matches.
  ConvGeom g = geom(C, H, W, kH, kW, hPadding, wPadding, yStride, xStride, xDilation, yDilation);
  if (int r = check_geom(g)) return r;
  // output size as the layer computes it (nConvolutionLayer.pas:92-100)
  const int64_t oh = out_dim(H, hPadding, kH, yDilation, yStride);
  const int64_t ow = out_dim(W, wPadding, kW, xDilation, xStride);
  const int64_t outImg = oh * ow, kSize = kH * kW, k = C * kSize;
  // with xDilation != yDilation the swapped im2col writes g.oh x g.ow columns
  // per row while the col buffer and the GEMM are sized for oh x ow: the
  // reference runs past its workspace there (or reads rows at the wrong
  // pitch); refused before any scratch is taken or anything is launched
  if (g.oh != oh || g.ow != ow)
    return set_error(TNS_ERR_UNSUPPORTED,
                     "conv2d: xDilation %lld, yDilation %lld give %lldx%lld im2col columns but "
                     "the layer's output is %lldx%lld (ntensors.pas:8303)",
                     (long long)xDilation, (long long)yDilation, (long long)g.oh,
                     (long long)g.ow, (long long)oh, (long long)ow);
  if (oh <= 0 || ow <= 0 || batch <= 0) return TNS_OK;
  const float* Bp;
  int64_t strideB;
  if (kSize != 1 || xDilation * yDilation != 1 || xStride * yStride != 1) {
    strideB = k * outImg;
    float* ws = workspace;
    if (!ws)
      if (int r = ensure_scratch(c, SLOT_COL, batch * strideB, &ws)) return r;
    {
      OpTimer t(c, TNS_OP_IM2COL);
      if (int r = hip_status(launch_im2col(g, input, C * H * W, ws, strideB, batch, c->stream),
                             "im2col launch"))
        return r;
    }
    Bp = ws;
  } else {
    strideB = C * H * W;
    Bp = input;
  }
  // one strided-batched launch with the weights shared (strideA = 0) — the
  // GPU path of nConvolutionLayer.pas:1078; beta = 0 as in Conv2D (8328)
  // The layer output is write-only here: beta = 0 does not read it (for any
  // finite previous contents this equals the reference's 0*C up to the sign
  // of an all-zero chain).
  return do_gemm(c, false, false, filters, outImg, k, 1.0f, weights, k, 0, Bp, outImg, strideB,
                 0.0f, out, outImg, outImg * filters, batch, EPI_NONE, nullptr, 0, true);
}

namespace {
struct ConvFwdOps {  // biases: null without the fused bias + activation
  const float *input, *weights, *biases;
  float *workspace, *out;
};

int activate_tail(tns_ctx* c, const ConvFwdPlan& p, const ConvFwdOps& o) {
  if (!p.act_tail) return TNS_OK;
  OpTimer t(c, TNS_OP_ACTIVATE);
  return hip_status(launch_activate(o.out, p.s.batch * p.s.filters * p.oh * p.ow, p.s.activation,
                                    c->stream),
                    "activate launch");
}

// the implicit-GEMM operands of images b0 .. b0 + nb, gathered from stored
// images of Hs x Ws (img floats each): mode 1 = zero-padded copies through
// the k-table kt, 2 = bounds-checked against a border of pad
GemmArgs conv_args(const ConvFwdPlan& p, const ConvFwdOps& o, const float* src, int64_t img,
                   int64_t Hs, int64_t Ws, int mode, const int* kt, int64_t pad, int64_t b0,
                   int64_t nb) {
  const int64_t outImg = p.oh * p.ow, k = p.s.C * p.s.kSize * p.s.kSize;
  GemmArgs a{};
  a.M = p.s.filters; a.N = nb * outImg; a.K = k;
  a.alpha = 1.0f; a.beta = 0.0f; a.beta_mode = BETA_ZERO;
  a.A = o.weights; a.lda = k; a.strideA = 0;
  a.B = src + b0 * img; a.ldb = outImg; a.strideB = img;
  a.C = o.out + b0 * outImg * p.s.filters; a.ldc = outImg; a.strideC = outImg * p.s.filters;
  a.batch = 1; a.epi = p.bias_act ? EPI_BIAS_ACT : EPI_NONE; a.bias = o.biases;
  a.act = p.epi_act;
  a.conv = mode; a.ktab = kt; a.ktab_n = kt ? (int)(k + KTAB_PAD) : 0;
  a.conv_H = (int)Hs; a.conv_W = (int)Ws; a.conv_ow = (int)p.ow; a.conv_ohw = (int)outImg;
  a.conv_sY = (int)p.s.stride; a.conv_sX = (int)p.s.stride;
  a.conv_pH = (int)pad; a.conv_pW = (int)pad;
  a.conv_bytes = (int)(4 * nb * img);
  return a;
}

int run_fwd_unfused(tns_ctx* c, const ConvFwdPlan& p, const ConvFwdOps& o) {
  const ConvShape& s = p.s;
  if (int r = tns_hip_conv2d(c, s.batch, s.C, s.H, s.W, o.input, o.weights, s.filters, s.kSize,
                             s.kSize, s.padding, s.padding, s.stride, s.stride, s.dilation,
                             s.dilation, o.workspace, o.out))
    return r;
  if (!p.bias_act) return TNS_OK;
  OpTimer t(c, TNS_OP_BIAS);
  return hip_status(launch_bias_activate(o.out, s.filters, p.oh * p.ow, o.biases, s.batch,
                                         s.activation, c->stream),
                    "bias+activate launch");
}

int run_fwd_direct(tns_ctx* c, const ConvFwdPlan& p, const ConvFwdOps& o) {
  const ConvShape& s = p.s;
  OpTimer t(c, TNS_OP_GEMM);
  return hip_status(launch_conv_direct(o.input, o.weights, o.biases, o.out, s.batch, s.C, s.H, s.W,
                                       s.filters, s.kSize, s.stride, s.padding, s.dilation, p.oh,
                                       p.ow, s.activation, c->stream),
                    "direct conv launch");
}

int run_fwd_conv1x1(tns_ctx* c, const ConvFwdPlan& p, const ConvFwdOps& o) {
  {
    OpTimer t(c, TNS_OP_GEMM);
    const hipError_t e = launch_conv1x1(p.form, o.weights, o.input, o.biases, o.out, p.s.batch,
                                        p.s.filters, p.s.C, p.oh * p.ow, p.epi_act, c->stream);
    if (e == hipErrorInvalidValue)
      return set_error(TNS_ERR_UNSUPPORTED, "conv1x1 form %d does not fit this layer", p.form);
    if (int r = hip_status(e, "conv1x1 launch")) return r;
  }
  return activate_tail(c, p, o);
}

int run_fwd_slab(tns_ctx* c, const ConvFwdPlan& p, const ConvFwdOps& o) {
  const ConvShape& s = p.s;
  float* slab = nullptr;
  if (int r = ensure_scratch(c, SLOT_COL, p.col_elems, &slab)) return r;
  ConvSlabArgs sa{};
  sa.input = o.input; sa.weights = o.weights; sa.bias = o.biases; sa.out = o.out;
  sa.batch = s.batch; sa.C = s.C; sa.H = s.H; sa.W = s.W; sa.M = s.filters;
  sa.K = s.C * s.kSize * s.kSize; sa.ks = s.kSize;
  sa.stride = s.stride; sa.pad = s.padding; sa.dil = s.dilation; sa.ow = p.ow; sa.ohw = p.oh * p.ow;
  sa.act = p.epi_act;
  {
    OpTimer t(c, TNS_OP_GEMM);
    const hipError_t e = launch_conv_slab(p.form, sa, slab, c->stream);
    if (e == hipErrorInvalidValue)
      return set_error(TNS_ERR_UNSUPPORTED, "conv slab form %d does not fit this layer", p.form);
    if (int r = hip_status(e, "conv slab launch")) return r;
  }
  return activate_tail(c, p, o);
}

int run_fwd_tile(tns_ctx* c, const ConvFwdPlan& p, const ConvFwdOps& o) {
  const ConvShape& s = p.s;
  for (int64_t b0 = 0; b0 < s.batch; b0 += p.chunk) {
    const GemmArgs a = conv_args(p, o, o.input, s.C * s.H * s.W, s.H, s.W, 2, nullptr, s.padding,
                                 b0, std::min(p.chunk, s.batch - b0));
    OpTimer t(c, TNS_OP_GEMM);
    const hipError_t e = launch_conv_tile(p.form, a, (int)s.kSize, (int)s.dilation, c->stream);
    if (e == hipErrorInvalidValue)
      return set_error(TNS_ERR_UNSUPPORTED, "conv tile %d does not fit this layer", p.form);
    if (int r = hip_status(e, "conv tile launch")) return r;
  }
  return activate_tail(c, p, o);
}

int run_fwd_implicit(tns_ctx* c, const ConvFwdPlan& p, const ConvFwdOps& o) {
  const ConvShape& s = p.s;
  const int64_t border = p.padded ? 2 * s.padding : 0;
  const int64_t Hs = s.H + border, Ws = s.W + border, img = s.C * Hs * Ws;
  const int* kt = nullptr;
  if (int r = get_ktab(c, s.C, Hs, Ws, s.kSize, s.kSize, s.dilation, s.dilation, &kt)) return r;
  const float* src = o.input;
  if (p.stage1_elems) {
    float* pbuf = nullptr;
    if (int r = ensure_scratch(c, SLOT_STAGE1, p.stage1_elems, &pbuf)) return r;
    OpTimer t(c, TNS_OP_IM2COL);
    if (int r = hip_status(launch_pad_images(o.input, s.batch, s.C, s.H, s.W, s.padding, s.padding,
                                             pbuf, c->stream), "pad launch"))
      return r;
    src = pbuf;
  }
  for (int64_t b0 = 0; b0 < s.batch; b0 += p.chunk) {
    const GemmArgs a = conv_args(p, o, src, img, Hs, Ws, p.padded ? 1 : 2, kt,
                                 p.padded ? 0 : s.padding, b0, std::min(p.chunk, s.batch - b0));
    OpTimer t(c, TNS_OP_GEMM);
    hipError_t e = launch_sgemm_conv_variant(p.form, a, c->stream);
    if (e == hipErrorInvalidValue)
      return set_error(TNS_ERR_UNSUPPORTED, "conv variant %lld unsupported",
                       (long long)p.conv_variant);
    if (int r = hip_status(e, "implicit conv launch")) return r;
  }
  return activate_tail(c, p, o);
}

int run_fwd_im2col(tns_ctx* c, const ConvFwdPlan& p, const ConvFwdOps& o) {
  const ConvShape& s = p.s;
  const int64_t outImg = p.oh * p.ow, k = s.C * s.kSize * s.kSize;
  const float* Bp = o.input;
  int64_t strideB = s.C * s.H * s.W;
  if (p.needs_col) {
    strideB = k * outImg;
    float* ws = o.workspace;
    if (!ws)
      if (int r = ensure_scratch(c, SLOT_COL, p.col_elems, &ws)) return r;
    OpTimer t(c, TNS_OP_IM2COL);
    const ConvGeom g = geom(s.C, s.H, s.W, s.kSize, s.kSize, s.padding, s.padding, s.stride,
                            s.stride, s.dilation, s.dilation);
    if (int r = hip_status(launch_im2col(g, o.input, s.C * s.H * s.W, ws, strideB, s.batch,
                                         c->stream), "im2col launch"))
      return r;
    Bp = ws;
  }
  // conv GEMM with forwardBias + activate fused into the epilogue
  if (int r = do_gemm(c, false, false, s.filters, outImg, k, 1.0f, o.weights, k, 0, Bp, outImg,
                      strideB, 0.0f, o.out, outImg, outImg * s.filters, s.batch,
                      p.bias_act ? EPI_BIAS_ACT : EPI_NONE, o.biases, p.epi_act, true))
    return r;
  return activate_tail(c, p, o);
}

// plan error, operands, the plan's path
int exec_conv_forward(tns_ctx* c, const ConvFwdPlan& p, const ConvFwdOps& o) {
  if (p.path == FWD_UNFUSED) return run_fwd_unfused(c, p, o);
  if (p.err && !p.implicit) return set_error(p.err, "%s", p.msg);
  if (p.implicit && (!o.input || !o.weights || !o.out || (p.bias_act && !o.biases)))
    return set_error(TNS_ERR_ARG, "conv_forward: null operand");
  if (p.err) return set_error(p.err, "%s", p.msg);
  switch (p.path) {
    case FWD_IM2COL: return run_fwd_im2col(c, p, o);
    case FWD_DIRECT: return run_fwd_direct(c, p, o);
    case FWD_CONV1X1: return run_fwd_conv1x1(c, p, o);
    case FWD_SLAB: return run_fwd_slab(c, p, o);
    case FWD_TILE: return run_fwd_tile(c, p, o);
    case FWD_IMPLICIT: return run_fwd_implicit(c, p, o);
    default: return TNS_OK;  // FWD_EMPTY
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

int tns_hip_conv_forward(tns_ctx* c, int64_t batch, int64_t C, int64_t H, int64_t W,
                         const float* input, const float* weights, const float* biases,
                         int64_t filters, int64_t kSize, int64_t stride, int64_t padding,
                         int64_t dilation, int32_t activation, float* workspace, float* out,
                         int32_t fused) {
  if (int r = check_ctx(c)) return r;
  if (!act_supported(activation))
    return set_error(TNS_ERR_UNSUPPORTED, "activation %d not implemented", activation);
  const ConvShape s{batch, C, H, W, filters, kSize, stride, padding, dilation, activation,
                    aligned16(weights)};
  return exec_conv_forward(c, plan_conv_forward(s, fused, true, g_opt),
                           ConvFwdOps{input, weights, biases, workspace, out});
}

int tns_hip_conv_forward_train(tns_ctx* c, int64_t batch, int64_t C, int64_t H, int64_t W,
                               const float* input, const float* weights, int64_t filters,
                               int64_t kSize, int64_t stride, int64_t padding, int64_t dilation,
                               int32_t activation, const float* scales, const float* biases,
                               float* rolling_mean, float* rolling_variance, float bnMomentum,
                               int32_t training, float* mean, float* variance, float* x,
                               float* x_norm, float* workspace, float* out) {
  if (int r = check_ctx(c)) return r;
  if (!act_supported(activation))
    return set_error(TNS_ERR_UNSUPPORTED, "activation %d not implemented", activation);
  if (!scales || !biases || !rolling_mean || !rolling_variance || !out ||
      (training && (!mean || !variance || !x || !x_norm)))
    return set_error(TNS_ERR_ARG, "conv_forward_train: null operand");
  const int64_t oh = out_dim(H, padding, kSize, dilation, stride);
  const int64_t ow = out_dim(W, padding, kSize, dilation, stride);
  if (oh <= 0 || ow <= 0 || batch <= 0 || filters <= 0) return TNS_OK;
  const int64_t bs = oh * ow;
  // state.input.Conv2D(weights, output, ...) (nConvolutionLayer.pas:508)
  const ConvShape s{batch, C, H, W, filters, kSize, stride, padding, dilation, activation,
                    aligned16(weights)};
  const ConvFwdPlan p = plan_conv_forward(s, TNS_CONV_FUSED, false, g_opt);
  if (int r = exec_conv_forward(c, p, ConvFwdOps{input, weights, nullptr, workspace, out}))
    return r;
  OpTimer t(c, TNS_OP_BIAS);
  if (!training)  // blockNormalize with the rolling statistics, scale, bias, activate
    return hip_status(launch_bn_apply(out, nullptr, nullptr, out, batch, filters, bs,
                                      rolling_mean, rolling_variance, scales, biases, activation,
                                      c->stream),
                      "batchNorm launch");
  float* part;
  if (int r = ensure_scratch(c, SLOT_BN, 2 * batch * filters, &part)) return r;
  if (int r = hip_status(launch_means_vars(out, batch, filters, bs, mean, variance, p.srss_quirk,
                                           part, c->stream),
                         "meansAndVars launch"))
    return r;
  if (int r = hip_status(launch_rolling_update(filters, rolling_mean, rolling_variance, mean,
                                               variance, bnMomentum, c->stream),
                         "rolling update launch"))
    return r;
  return hip_status(launch_bn_apply(out, x, x_norm, out, batch, filters, bs, mean, variance,
                                    scales, biases, activation, c->stream),
                    "batchNorm launch");
}

// ---- backward ------------------------------------------------------------------
namespace {
struct ConvBN {  // batchNormBack operands (nbaselayer.pas:372-395); scales == nullptr: none
  const float *scales, *x, *x_norm, *mean, *variance;
  float *scale_updates, *mean_delta, *variance_delta;
};
struct ConvBwdOps {
  const float *input, *weights, *output;
  float *delta, *bias_updates, *weight_updates, *workspace, *state_delta;
  ConvBN bn;
};
// what the call holds once its scratch is acquired
struct ConvBwdRun {
  bool pipe = false, overlap = false;
  const ConvDwChoice* dw = nullptr;  // the plan's choice, or its fall-back
  DwResArgs dres{};                  // residue scratch
  float* part = nullptr;             // SLOT_BN
  float* ws = nullptr;               // dW's col buffer
  float* dx_ws = nullptr;            // col buffer of state.delta's chain
  float* wt = nullptr;               // SLOT_WT
};

// Derivative() and the bias / batch-norm terms of delta, before dW and dX
int run_bwd_prologue(tns_ctx* c, const ConvBwdPlan& p, const ConvBwdOps& o, float* part) {
  const ConvBN& bn = o.bn;
  const int64_t batch = p.s.batch, filters = p.s.filters, i_k = p.i_k;
  const int act = p.s.activation;
  float* delta = o.delta;
  hipError_t fe = hipErrorNotSupported;
  if (p.bn_fused)
    fe = launch_bn_backward_fused(bn.scale_updates, bn.x_norm, delta, o.output, act, bn.x, bn.mean,
                                  bn.variance, bn.scales, bn.mean_delta, bn.variance_delta, batch,
                                  filters, i_k, p.srss_quirk, part, c->stream);
  if (fe != hipErrorNotSupported) return hip_status(fe, "batchNormBack launch");
  if (p.has_bn) {
    // Derivative(): delta *= f'(output), then batchNormBack:
    // scale_updates.addDots(x_norm, delta); delta.forwardScale(scales);
    // MeansAndVarsDelta; normalizeDelta — and no bias_updates term
    // (nConvolutionLayer.pas:601-604).  Three passes instead of five: the
    // derive rides addDots' loads (each derived term written back), and the
    // scale is applied to each delta term as MeansAndVarsDelta and
    // normalizeDelta load it (the same one rounding forwardScale would store)
    if (int r = hip_status(launch_add_dots_derive(bn.scale_updates, bn.x_norm, delta, o.output, act,
                                                  batch, filters, i_k, part, c->stream),
                           "derive + addDots launch"))
      return r;
    const float* fold = bn_folds_scale(i_k) ? bn.scales : nullptr;
    if (!fold)
      if (int r = hip_status(launch_scale_add(delta, batch, filters, i_k, bn.scales, nullptr, 1,
                                              c->stream), "forwardScale launch"))
        return r;
    if (int r = hip_status(launch_mean_var_delta(delta, bn.x, bn.mean, bn.variance, batch, filters,
                                                 i_k, bn.mean_delta, bn.variance_delta,
                                                 p.srss_quirk, part, c->stream, fold),
                           "meansAndVarsDelta launch"))
      return r;
    return hip_status(launch_normalize_delta(bn.x, bn.mean, bn.variance, bn.mean_delta,
                                             bn.variance_delta, delta, batch, filters, i_k,
                                             c->stream, fold), "normalizeDelta launch");
  }
  // Derivative(): delta *= f'(output), then bias_updates.addSums(delta) —
  // one pass (each derived term written back as it enters the sums' chains)
  if (p.derive_sums)
    return hip_status(launch_derive_add_sums(o.bias_updates, delta, o.output, act, batch, filters,
                                             i_k, part, c->stream),
                      "derive + addSums launch");
  if (int r = hip_status(launch_derive(o.output, batch * filters * i_k, act, delta, c->stream),
                         "derive launch"))
    return r;
  return hip_status(launch_add_sums(o.bias_updates, delta, batch, filters, i_k, part, c->stream),
                    "addSums launch");
}

// every scratch buffer of dW and dX, sized before any fork (a growth inside
// the side-stream chain would free a buffer the main stream may use), and
// the schedule the context can run: r.pipe (in: the pipelined schedule was
// entered) and r.overlap
int acquire_bwd_scratch(tns_ctx* c, const ConvBwdPlan& p, const ConvBwdOps& o, ConvBwdRun& r) {
  r.dw = &p.dw;
  // the residue form's scratch; when the form was picked by shape and that
  // memory cannot be had, the dW falls back to the paths that need only the
  // workspace (dw_tile, or im2col + the sdot kernels)
  if (p.dw.path == DW_RES) {
    int e = ensure_scratch(c, SLOT_RES_A, p.res_a_elems, &r.dres.dA, r.pipe);
    if (!e) e = ensure_scratch(c, SLOT_RES_B, p.res_b_elems, &r.dres.dB, r.pipe);
    if (!e) e = ensure_scratch(c, SLOT_DW, p.dw.part_elems, &r.dres.part, r.pipe);
    if (e) {
      if (p.dw_res_forced) return e;  // (forced: the error stands)
      tns_clear_error();
      release_scratch(c, SLOT_RES_A);
      release_scratch(c, SLOT_RES_B);
      r.dw = &p.dw_fallback;
    }
  }
  // dW (im2col + sdot or dw_tile, accumulate) and state.delta (TN + col2im
  // or the fused kernel) read delta and write disjoint outputs: with a
  // state.delta they run concurrently, state.delta's chain on the context's
  // side stream (fork / join events), each with its own col buffer —
  // nothing changes in either result.  Telemetry times ops one by one, so it
  // keeps them in sequence.
  r.overlap = !r.pipe && p.has_state_delta && p.sched != BWD_SEQUENTIAL && !c->telemetry &&
              ensure_side_stream(c);
  // state.delta's own col buffer when both chains need one at once (the
  // overlap's extra memory, tns.h); if it cannot be had, the sequential
  // schedule shares the one col buffer instead
  if (r.overlap && r.dw->col && p.dx_col &&
      ensure_scratch(c, SLOT_COL_DX, p.col_elems, &r.dx_ws)) {
    tns_clear_error();
    r.overlap = false;
  }
  // (pipelined: state.delta's chain always has its own col buffer — the
  // pending dW products may still read the shared one)
  // (if that buffer cannot be had: the pending dW joined, this call in
  // sequence within the caller's workspace)
  if (r.pipe && p.dx_col && ensure_scratch(c, SLOT_COL_DX, p.col_elems, &r.dx_ws)) {
    tns_clear_error();
    r.dx_ws = nullptr;
    r.pipe = false;
    if (int e = join_side(c)) return e;
  }
  r.ws = o.workspace;
  if (!r.ws && (r.dw->col || (p.dx_col && !r.dx_ws && !(r.overlap && r.dw->col))))
    if (int e = ensure_scratch(c, SLOT_COL, p.col_elems, &r.ws, r.pipe)) return e;
  if (!r.dx_ws) r.dx_ws = r.ws;
  // scratch of the fused state.delta kernel / the transposed weights
  if (p.wt_elems)
    if (int e = ensure_scratch(c, SLOT_WT, p.wt_elems, &r.wt)) return e;
  return TNS_OK;
}

int run_dw(tns_ctx* c, const ConvBwdPlan& p, const ConvBwdOps& o, const ConvBwdRun& r) {
  const ConvShape& s = p.s;
  const int64_t batch = s.batch, i_m = p.i_m, i_n = p.i_n, i_k = p.i_k;
  const ConvDwChoice& dw = *r.dw;
  if (dw.path == DW_RES) {
    DwResArgs d = r.dres;
    d.g = p.g;
    d.x = o.input; d.xStride = s.C * s.H * s.W;
    d.delta = o.delta; d.weight_updates = o.weight_updates;
    d.M = i_m; d.N = i_n; d.K = i_k; d.batch = batch;
    d.direct = !p.needs_col; d.alpha = 1.0f;
    OpTimer t(c, TNS_OP_GEMM);
    const hipError_t e = launch_dw_res(dw.form, d, c->stream);
    if (e == hipErrorInvalidValue)
      return set_error(TNS_ERR_UNSUPPORTED, "dW res form %d does not fit this layer", dw.form);
    return hip_status(e, "dW res launch");
  }
  float* part = nullptr;
  if (dw.path == DW_TILE) {
    if (int e = ensure_scratch(c, SLOT_DW, dw.part_elems, &part, r.pipe)) return e;
    DwArgs da = dw_tile_args(p, o.delta, o.input);
    da.part = part;
    {
      OpTimer t(c, TNS_OP_GEMM);
      const hipError_t e = launch_dw_tile(dw.form, da, (int)s.kSize, c->stream);
      if (e == hipErrorInvalidValue)
        return set_error(TNS_ERR_UNSUPPORTED, "dW tile %d does not fit this layer", dw.form);
      if (int e2 = hip_status(e, "dW tile launch")) return e2;
    }
    return hip_status(launch_add_in_order(o.weight_updates, part, i_m * i_n, batch, c->stream),
                      "dW accumulate launch");
  }
  const float* col = o.input;
  if (p.needs_col) {
    OpTimer t(c, TNS_OP_IM2COL);
    if (int e = hip_status(launch_im2col(p.g, o.input, s.C * s.H * s.W, r.ws, p.colSize, batch,
                                         c->stream), "im2col launch"))
      return e;
    col = r.ws;
  }
  // weight_updates += delta_b . col_b^T, one NT GEMM per image (beta = 1),
  // in image order as the reference loop (nConvolutionLayer.pas:636-640):
  // each image adds sum_b = 1*sdot(...) to C.  The sums of different images
  // are independent, so they are computed by ONE strided-batched sdot launch
  // (each stored as is, BETA_STORE), then added to C image by image in the
  // reference's order — the same roundings, batch-fold more parallelism for
  // the few-tile, long-k dW shapes.
  if (dw.path == DW_SDOT) {
    if (int e = ensure_scratch(c, SLOT_DW, dw.part_elems, &part, r.pipe)) return e;
    GemmArgs a{};
    a.M = i_m; a.N = i_n; a.K = i_k;
    a.alpha = 1.0f; a.beta = 0.0f; a.beta_mode = BETA_STORE;
    a.A = o.delta; a.lda = i_k; a.strideA = i_m * i_k;
    a.B = col; a.ldb = i_k; a.strideB = p.colSize;
    a.C = part; a.ldc = i_n; a.strideC = i_m * i_n;
    a.batch = batch; a.epi = EPI_NONE;
    {
      OpTimer t(c, TNS_OP_GEMM);
      if (int e = hip_status(launch_sgemm_nt_sdot(a, c->stream), "sgemm_nt launch")) return e;
    }
    return hip_status(launch_add_in_order(o.weight_updates, part, i_m * i_n, batch, c->stream),
                      "dW accumulate launch");
  }
  for (int64_t b = 0; b < batch; ++b)
    if (int e = do_gemm(c, false, true, i_m, i_n, i_k, 1.0f, o.delta + b * i_m * i_k, i_k, 0,
                        col + b * p.colSize, i_k, 0, 1.0f, o.weight_updates, i_n, 0, 1, EPI_NONE,
                        nullptr, 0))
      return e;
  return TNS_OK;
}

int run_dx(tns_ctx* c, const ConvBwdPlan& p, const ConvBwdOps& o, const ConvBwdRun& r) {
  const ConvShape& s = p.s;
  const int64_t batch = s.batch, C = s.C, H = s.H, W = s.W, filters = s.filters, kSize = s.kSize;
  const int64_t i_m = p.i_m, i_n = p.i_n, i_k = p.i_k;
  if (p.dx == DX_FUSED) {
    // per image pixel: each window tap's ascending-f chain, added to the
    // pixel in (kr, kc) order for the taps scol2im does not skip — the same
    // roundings as the two stages below (646-660)
    OpTimer t(c, TNS_OP_GEMM);
    return hip_status(launch_conv_dx_col2im(o.weights, r.wt, o.delta, o.state_delta, batch, C, H,
                                            W, filters, kSize, s.padding, s.dilation, p.g.oh,
                                            p.g.ow, c->stream),
                      "fused dX + col2im launch");
  }
  if (p.dx == DX_CONV3 || p.dx == DX_CONV3S2) {
    const bool s2 = p.dx == DX_CONV3S2;
    OpTimer t(c, TNS_OP_GEMM);
    if (int e = hip_status(
            s2 ? launch_transpose_taps(o.weights, r.wt, filters, C, kSize * kSize, c->stream,
                                       conv_tile4_dx3s2_order(s.padding))
               : launch_transpose_taps(o.weights, r.wt, filters, C, kSize * kSize, c->stream),
            "weights transpose launch"))
      return e;
    const hipError_t e =
        s2 ? launch_conv_tile4_dx3s2(p.dx_form, r.wt, o.delta, o.state_delta, batch, C, H, W,
                                     filters, s.padding, p.g.oh, p.g.ow, c->stream)
           : launch_conv_tile4_dx3(p.dx_form, r.wt, o.delta, o.state_delta, batch, C, H, W,
                                   filters, kSize, s.padding, p.g.oh, p.g.ow, c->stream);
    if (e != hipErrorInvalidValue) return hip_status(e, "dX conv launch");
    return set_error(TNS_ERR_UNSUPPORTED, "dX conv form %d does not fit this layer", p.dx_form);
  }
  // col_b = W^T . delta_b (TN strided batched, weights shared, beta = 0 into
  // the workspace), then col2im accumulates into state.delta (646-660).  All
  // images in one launch on conv_tile4's k-major-A forms where they apply (a
  // 1x1 "convolution" over the delta planes, the same chains), else the TN
  // GEMM
  bool done = false;
  float* col = p.dx_direct ? o.state_delta : r.dx_ws;
  if (p.dx == DX_CONV1X1) {  // (1x1 / stride 1: dx_direct)
    OpTimer t(c, TNS_OP_GEMM);
    if (int e = hip_status(launch_transpose(o.weights, r.wt, filters, C, c->stream),
                           "weights transpose launch"))
      return e;
    const hipError_t e = launch_conv1x1(p.dx_form, r.wt, o.delta, nullptr, o.state_delta, batch, C,
                                        filters, i_k, 0, c->stream, true);
    if (e == hipSuccess) return TNS_OK;
    if (e != hipErrorInvalidValue) return hip_status(e, "dX 1x1 launch");
    // (operands off the 16-byte alignment the DMA needs: the TN product)
  }
  if (p.dx_tile >= 0) {
    OpTimer t(c, TNS_OP_GEMM);
    const hipError_t e = launch_conv_tile4_dx(p.dx_tile, o.weights, o.delta, col, batch, C, kSize,
                                              filters, p.g.oh, p.g.ow, c->stream, p.dx_direct);
    if (e == hipSuccess)
      done = true;
    else if (e != hipErrorInvalidValue || p.dx_tile_forced)
      return e == hipErrorInvalidValue
                 ? set_error(TNS_ERR_UNSUPPORTED, "dX tile %d does not fit this layer", p.dx_tile)
                 : hip_status(e, "dX tile launch");
  }
  if (!done)
    if (int e = do_gemm(c, true, false, i_n, i_k, i_m, 1.0f, o.weights, i_n, 0, o.delta, i_k,
                        i_m * i_k, 0.0f, col, i_k, p.colSize, batch,
                        p.dx_direct ? EPI_ADD : EPI_NONE, nullptr, 0, true))
      return e;
  if (p.dx_direct) return TNS_OK;
  OpTimer t(c, TNS_OP_COL2IM);
  return hip_status(launch_col2im(p.g, r.dx_ws, p.colSize, o.state_delta, C * H * W, batch,
                                  c->stream),
                    "col2im launch");
}

// dW enqueued on the side stream behind the earlier calls' (fork: after
// this call's derive / bias sums), state.delta's chain on the context's
// stream; no join — the side stream's work is joined by the next call of
// any other entry point (tns.h TNS_OPT_BWD_OVERLAP)
int run_bwd_pipelined(tns_ctx* c, const ConvBwdPlan& p, const ConvBwdOps& o, const ConvBwdRun& r) {
  const ConvShape& s = p.s;
  TNS_HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
  TNS_HIP_TRY(hipStreamWaitEvent(c->aux_stream, c->ev_fork, 0));
  hipStream_t main = c->stream;
  c->home_stream = main;
  c->stream = c->aux_stream;
  const int rw = run_dw(c, p, o, r);
  c->stream = main;
  c->home_stream = nullptr;
  c->side_pending = true;
  // the record of this dW's operands and of the scratch slots it uses
  // (kept after a failed launch too: whatever it enqueued stays ordered)
  tns_ctx::PendingDw d;
  const Span rd = span(o.delta, s.batch * s.filters * p.i_k);
  const Span ri = span(o.input, s.batch * s.C * s.H * s.W);
  const Span wu = span(o.weight_updates, p.i_m * p.i_n);
  const Span wc = r.dw->col && r.ws == o.workspace ? span(r.ws, s.batch * p.colSize) : Span{};
  d.lo[0] = rd.lo; d.hi[0] = rd.hi;
  d.lo[1] = ri.lo; d.hi[1] = ri.hi;
  d.wlo[0] = wu.lo; d.whi[0] = wu.hi;
  d.wlo[1] = wc.lo; d.whi[1] = wc.hi;
  c->pending.push_back(d);
  c->side_slots |= 1u << SLOT_RES_A | 1u << SLOT_RES_B | 1u << SLOT_DW |
                   (r.dw->col && r.ws != o.workspace ? 1u << SLOT_COL : 0u);
  if (rw) return rw;
  return o.state_delta ? run_dx(c, p, o, r) : TNS_OK;
}

// state.delta's chain on the overlap stream beside the dW on the context's,
// joined before the call returns
int run_bwd_joined(tns_ctx* c, const ConvBwdPlan& p, const ConvBwdOps& o, const ConvBwdRun& r) {
  TNS_HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
  TNS_HIP_TRY(hipStreamWaitEvent(c->ovl_stream, c->ev_fork, 0));
  // (every launch inside run_dx goes to c->stream)
  hipStream_t main = c->stream;
  c->stream = c->ovl_stream;
  const int rx = run_dx(c, p, o, r);
  c->stream = main;
  // joined even after an error, so later work on the stream stays ordered
  const hipError_t ej = hipEventRecord(c->ev_join, c->ovl_stream);
  const int rw = run_dw(c, p, o, r);
  const hipError_t ew = ej == hipSuccess ? hipStreamWaitEvent(c->stream, c->ev_join, 0) : ej;
  if (rx) return rx;
  if (rw) return rw;
  return hip_status(ew, "backward join");
}

// TConvolutionalLayer.backward: plan, report, acquire scratch, run, schedule
int conv_backward(tns_ctx* c, const ConvShape& s, const ConvBwdOps& o) {
  // (pipelined mode: this call's dW queues behind the pending ones on the
  // side stream; its other work touches none of their operands)
  if (!c) return check_ctx(c);
  const ConvBN& bn = o.bn;
  const ConvBwdPlan p = plan_conv_backward(s, bn.scales != nullptr, o.state_delta != nullptr,
                                           aligned16(o.delta), g_opt);
  ConvBwdRun r;
  r.pipe = p.sched == BWD_PIPELINED && !c->telemetry && ensure_side_stream(c);
  if (int e = check_ctx(c, !r.pipe)) return e;
  if (!act_supported(s.activation))
    return set_error(TNS_ERR_UNSUPPORTED, "activation %d not implemented", s.activation);
  if (p.err) return set_error(p.err, "%s", p.msg);
  if (p.empty) return TNS_OK;
  if (!o.input || !o.weights || !o.output || !o.delta || !o.weight_updates ||
      (!bn.scales && !o.bias_updates))
    return set_error(TNS_ERR_ARG, "conv_backward: null operand");
  if (bn.scales && (!bn.x || !bn.x_norm || !bn.mean || !bn.variance || !bn.scale_updates ||
                    !bn.mean_delta || !bn.variance_delta))
    return set_error(TNS_ERR_ARG, "conv_backward: null batch-norm operand");
  if (r.pipe) {
    // this call writes delta (in place) and state.delta on the context's
    // stream: if a pending dW reads either (an earlier call on the same
    // layers, e.g. the previous pass), the side stream is joined first (no
    // per-call event: the join is only paid where the ranges meet)
    // (the same test as every other entry point's, over this call's
    // context-stream operands; its own dW queues on the side stream)
    const int64_t nf = bn.scales ? s.filters : 0, nd = s.batch * s.filters * p.i_k;
    if (int e = check_ops(c,
                          {span(o.delta, nd), span(o.state_delta, s.batch * s.C * s.H * s.W),
                           span(o.bias_updates, bn.scales ? 0 : s.filters),
                           span(bn.scale_updates, nf), span(bn.mean_delta, nf),
                           span(bn.variance_delta, nf)},
                          {span(o.output, nd), span(o.weights, s.filters * p.i_n),
                           span(bn.x, nf ? nd : 0), span(bn.x_norm, nf ? nd : 0),
                           span(bn.scales, nf), span(bn.mean, nf), span(bn.variance, nf)}))
      return e;
  }
  if (int e = ensure_scratch(c, SLOT_BN, p.bn_elems, &r.part)) return e;
  if (int e = run_bwd_prologue(c, p, o, r.part)) return e;
  if (int e = acquire_bwd_scratch(c, p, o, r)) return e;
  if (r.pipe) return run_bwd_pipelined(c, p, o, r);
  if (r.overlap) return run_bwd_joined(c, p, o, r);
  if (int e = run_dw(c, p, o, r)) return e;
  return o.state_delta ? run_dx(c, p, o, r) : TNS_OK;
}
}  // namespace

int tns_hip_conv_backward(tns_ctx* c, int64_t batch, int64_t C, int64_t H, int64_t W,
                          const float* input, const float* weights, int64_t filters,
                          int64_t kSize, int64_t stride, int64_t padding, int64_t dilation,
                          int32_t activation, const float* output, float* delta,
                          float* bias_updates, float* weight_updates, float* workspace,
                          float* state_delta) {
  return conv_backward(c, ConvShape{batch, C, H, W, filters, kSize, stride, padding, dilation,
                                    activation, false},
                       ConvBwdOps{input, weights, output, delta, bias_updates, weight_updates,
                                  workspace, state_delta, ConvBN{}});
}

int tns_hip_conv_backward_bn(tns_ctx* c, int64_t batch, int64_t C, int64_t H, int64_t W,
                             const float* input, const float* weights, int64_t filters,
                             int64_t kSize, int64_t stride, int64_t padding, int64_t dilation,
                             int32_t activation, const float* output, float* delta,
                             const float* scales, const float* x, const float* x_norm,
                             const float* mean, const float* variance, float* scale_updates,
                             float* mean_delta, float* variance_delta, float* weight_updates,
                             float* workspace, float* state_delta) {
  if (!scales) return set_error(TNS_ERR_ARG, "conv_backward_bn: null scales");
  ConvBN bn{scales, x, x_norm, mean, variance, scale_updates, mean_delta, variance_delta};
  return conv_backward(c, ConvShape{batch, C, H, W, filters, kSize, stride, padding, dilation,
                                    activation, false},
                       ConvBwdOps{input, weights, output, delta, nullptr, weight_updates,
                                  workspace, state_delta, bn});
}

// ---- the forms TNS_OPT_CONV_VARIANT / DX_TILE / DX_CONV / DW_RES / DW_TILE index ----
int tns_conv_tile_variant_count(void) { return conv_tile_count(); }
int tns_conv_slab_count(void) { return conv_slab_count(); }
int tns_conv1x1_count(void) { return conv1x1_count(); }
const char* tns_conv1x1_name(int32_t v) { return conv1x1_name(v); }
const char* tns_conv_slab_name(int32_t v) { return conv_slab_name(v); }
int tns_conv_dx_tile_count(void) { return conv_tile4_ta_count(); }
int tns_conv_dx_conv_count(void) { return conv_tile4_dx3_count(); }
int tns_conv_dw_res_count(void) { return dw_res_count(); }
int tns_conv_dw_tile_count(void) { return dw_tile_count(); }
const char* tns_conv_tile_variant_name(int32_t v) { return conv_tile_name(v); }
