// conv_bf16_bwd.hip — the convolution backward's two products on the bf16 MFMA
// (v_mfma_f32_32x32x16_bf16), the opt-in reduced-precision training path
// ("bf16 conv backward").  Operands are rounded to bf16 (nearest
// even) on their way into the MFMA; products are exact in fp32, accumulated in
// fp32 and added to the fp32 buffers.  No atomics: the same call gives the
// same bits.  Dilation 1 only, as in the forward (conv_bf16.hip), whose LDS row
// geometry, fragment reads and MFMA schedule both kernels keep.
//
// dX  state_delta += W^T (*) delta, one implicit GEMM: M = C, N = batch * H * W
//     (input pixels, the batch folded into the columns), K = filters * k * k in
//     (f, ky, kx) order.
//   A  the transposed weights A[c][(f, ky, kx)] = W[f][(c, ky, kx)], rounded
//      and packed per call by conv_bf16_pack_wt_kernel in the forward's
//      A-fragment order; a wave reads its fragments straight into registers,
//      one step ahead.
//   B  gathered from the fp32 delta through the k-table of a (filters, oh, ow)
//      image (plane offset and tap per k, wave-uniform): for the column
//      (b, iy, ix) and k = (f, ky, kx), ty = iy + pad - ky, tx = ix + pad - kx;
//      the element is delta[b][f][ty / s][tx / s] where ty, tx >= 0, both are
//      multiples of the stride s and ty / s < oh, tx / s < ow, else zero.  Every
//      load is inside the tensor (an outside tap reads element 0 and is
//      replaced).  At stride 2 three taps in four are such zeros and still pass
//      through the MFMA.
//   C  the forward's two tiles (128 x 128, 64 x 64); the epilogue is
//      state_delta[b][c][iy][ix] += acc, each element owned by one thread.
//
// dW  weight_updates += sum_b delta_b . col_b^T, a GEMM whose reduction is the
//     long dimension: M = filters, N = K = C * k * k in (c, ky, kx) order, the
//     reduction r = b * oh * ow + p over R = batch * oh * ow, in steps of 32.
//   A  the fp32 delta, row f, contiguous in p inside an image.
//   B  gathered from the fp32 input: row n = (c, ky, kx) of the forward's
//      k-table, element input[b][c][oy * s - pad + ky][ox * s - pad + kx], the
//      window bounds checked, zeros outside.
//      A thread owns one 8-piece (8 consecutive r) of T rows of each operand:
//      it decodes (b, oy, ox) of the piece's first r once a step and carries
//      them element by element over row and image ends (a step may straddle
//      images), rounds the eight floats to four bf16 pairs in registers and
//      writes one 16-byte piece to LDS, r-contiguous per row, 64 bytes of data
//      in a row of 80: the fragment reads of both operands are the forward's
//      B reads.  Rows past filters or K and r past R contribute zeros.
//   split  the reduction is cut into S contiguous slices of steps
//      (conv_bf16_dw_split); slice sl of a tile writes its fp32 partial tile to
//      scratch [S][filters][K], and conv_bf16_dw_sum_kernel adds the slices in
//      the order 0 .. S-1 and then the total to weight_updates.  With S = 1 the
//      main kernel adds into weight_updates itself.
#include <algorithm>

#include "tns_internal.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "conv_bf16_common.hpp"

namespace tns {
namespace {

using namespace bf16k;

// ---- dX ------------------------------------------------------------------------
struct DxArgs {
  const float* delta;
  const uint4* packed;
  float* sd;
  const int* ktab;
  int64_t N, dimg, simg;  // columns; floats a delta image; floats a state_delta image
  int ktab_n, W, HW, oh, ow, stride, sshift, pad, C;
  int steps, ks16, mtiles;  // K / 32, K / 16 (padded K), tiles over the channels
};

// W^T rounded into the forward's A-fragment order: one thread per 16-byte
// piece; row c, k = (f, ky, kx) reads w[f][c][ky][kx]
__global__ void __launch_bounds__(kThreads)
conv_bf16_pack_wt_kernel(int64_t pieces, int C, int filters, int kk, int ks16,
                         const float* __restrict__ w, uint4* __restrict__ packed) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= pieces) return;
  const int lane = (int)(q & 63);
  const int64_t frag = q >> 6;
  const int ks = (int)(frag % ks16);
  const int64_t c = (frag / ks16) * 32 + (lane & 31);
  const int k0 = ks * 16 + 8 * (lane >> 5);
  const int Kd = filters * kk;
  int f = k0 / kk, t = k0 - f * kk;
  unsigned v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = (c < C && k0 + i < Kd) ? bf16_rne(w[((int64_t)f * C + c) * kk + t]) : 0u;
    if (++t == kk) t = 0, ++f;
  }
  packed[q] = make_uint4(v[0] | v[1] << 16, v[2] | v[3] << 16, v[4] | v[5] << 16,
                         v[6] | v[7] << 16);
}

// a thread's input pixel: its delta image and iy + pad, ix + pad (a column
// past N: a row no tap brings inside the delta plane)
struct DxColumn {
  const float* img;
  int ty0, tx0;
};

// KPT consecutive k for the thread's column, every load inside the image
template <int KPT>
__device__ __forceinline__ void gather_dx(const DxArgs& a, const DxColumn& c, int k0,
                                          float (&g)[KPT]) {
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const int off = a.ktab[k0 + i], win = a.ktab[a.ktab_n + k0 + i];
    const int ky = win & 0xffff, kx = win >> 16;
    const int plane = (off >> 2) - ky * a.ow - kx;  // f * oh * ow
    const int ty = c.ty0 - ky, tx = c.tx0 - kx;
    int qy, qx;
    bool ok;
    if (a.sshift >= 0) {
      qy = ty >> a.sshift, qx = tx >> a.sshift;
      ok = ((ty | tx) & (a.stride - 1)) == 0;
    } else {
      qy = ty / a.stride, qx = tx / a.stride;
      ok = qy * a.stride == ty && qx * a.stride == tx;
    }
    ok = ok && (ty | tx) >= 0 && qy < a.oh && qx < a.ow;
    const float x = c.img[ok ? plane + qy * a.ow + qx : 0];
    g[i] = ok ? x : 0.0f;
  }
}

// grid: mtiles * column tiles, the channel tiles of one column tile side by side
template <int TM, int TN>
__global__ void __launch_bounds__(kThreads) conv_bf16_dx_kernel(const DxArgs a) {
  constexpr int BN = 64 * TN, KPT = BN / 8;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][BN * kRow];
  const int tid = threadIdx.x, lane = tid & 63, lc = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int mt = blockIdx.x % a.mtiles;
  const int64_t n0 = (int64_t)(blockIdx.x / a.mtiles) * BN;

  const int gp = tid % BN;
  const int gk = __builtin_amdgcn_readfirstlane(tid / BN) * KPT;
  DxColumn col{a.delta, -0x8000, 0};
  if (n0 + gp < a.N) {
    const int64_t b = (n0 + gp) / a.HW;
    const int p = (int)(n0 + gp - b * a.HW);
    const int iy = p / a.W;
    col.ty0 = iy + a.pad;
    col.tx0 = p - iy * a.W + a.pad;
    col.img = a.delta + b * a.dimg;
  }
  unsigned char* const wrow = &lds[0][0] + gp * kRow + gk * 2;

  const uint4* ap[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
    ap[i] = a.packed + (int64_t)(mt * 2 * TM + wm * TM + i) * a.ks16 * 64 + lane;
  const unsigned char* const rrow = &lds[0][0] + (wn * 32 * TN + lc) * kRow + h * 16;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  float g[KPT];
  uint4 ac[TM][2], an[TM][2];
  gather_dx<KPT>(a, col, gk, g);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    ac[i][0] = ap[i][0];
    ac[i][1] = ap[i][64];
  }
  store_b<KPT>(wrow, g);
  __syncthreads();

  for (int s = 0; s < a.steps; ++s) {
    const bool more = s + 1 < a.steps;
    if (more) {
      gather_dx<KPT>(a, col, (s + 1) * kStep + gk, g);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        an[i][0] = ap[i][(2 * s + 2) * 64];
        an[i][1] = ap[i][(2 * s + 3) * 64];
      }
    }
    const unsigned char* const rb = rrow + (s & 1) * (BN * kRow);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      bf16x8 bf[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j)
        bf[j] = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const uint4*>(rb + j * 32 * kRow + hh * 32));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              __builtin_bit_cast(bf16x8, ac[i][hh]), bf[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      store_b<KPT>(wrow + ((s + 1) & 1) * (BN * kRow), g);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        ac[i][0] = an[i][0];
        ac[i][1] = an[i][1];
      }
    }
    __syncthreads();
  }

  // epilogue: col2im accumulates, so state_delta += acc (32 consecutive pixels a row)
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int64_t n = n0 + wn * 32 * TN + j * 32 + lc;
    const bool inside = n < a.N;
    const int64_t b = inside ? n / a.HW : 0;
    float* const o = a.sd + b * a.simg + (n - b * a.HW);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int c0 = (mt * 2 * TM + wm * TM + i) * 32 + 4 * h;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int c = c0 + (e & 3) + 8 * (e >> 2);
        if (inside && c < a.C) o[(int64_t)c * a.HW] += acc[i][j][e];
      }
    }
  }
}

// ---- dW ------------------------------------------------------------------------
struct Bf16DwArgs {
  const float* delta;
  const float* in;
  float* out;  // weight_updates, or the partials [S][filters][K]
  const int* ktab;
  int64_t chw, dimg;  // floats an input image; floats a delta image
  int ktab_n, R, ohw, oh, ow, H, W, stride, pad, filters, K;
  int steps, per, mtiles, ntiles, partial;  // reduction steps; steps a slice
};

// the thread's 8-piece of reduction step s: T rows of delta and T rows of the
// implicit im2col matrix, eight consecutive r each
template <int T>
__device__ __forceinline__ void gather_dw(const Bf16DwArgs& a, int s, int q, const int (&frow)[T],
                                          const int (&boff)[T], const int (&bwin)[T],
                                          float (&ga)[T][8], float (&gb)[T][8]) {
  const int r0 = s * kStep + q * 8;
  int b = r0 / a.ohw;
  int p = r0 - b * a.ohw;
  int oy = p / a.ow, ox = p - oy * a.ow;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const bool valid = r0 + e < a.R;
    const int iy0 = oy * a.stride - a.pad, ix0 = ox * a.stride - a.pad;
    const int64_t dimg = (int64_t)b * a.dimg + p;
    const int64_t iimg = (int64_t)b * a.chw + iy0 * a.W + ix0;
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const bool oka = valid && frow[j] >= 0;
      const float d = a.delta[oka ? dimg + frow[j] : 0];
      ga[j][e] = oka ? d : 0.0f;
      const int iy = iy0 + (bwin[j] & 0xffff), ix = ix0 + (bwin[j] >> 16);
      const bool okb = valid && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      const float x = a.in[okb ? iimg + boff[j] : 0];
      gb[j][e] = okb ? x : 0.0f;
    }
    ++p;
    if (++ox == a.ow) {
      ox = 0;
      if (++oy == a.oh) oy = 0, p = 0, ++b;
    }
  }
}

// grid: tiles * slices; a block's 2 x 2 waves hold T x T MFMA tiles each
template <int T>
__global__ void __launch_bounds__(kThreads) conv_bf16_dw_kernel(const Bf16DwArgs a) {
  constexpr int BT = 64 * T, kBuf = BT * kRow;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][kBuf];  // [stage][A, B]
  const int tid = threadIdx.x, lane = tid & 63, lc = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int tiles = a.mtiles * a.ntiles;
  const int tile = blockIdx.x % tiles, sl = blockIdx.x / tiles;
  const int m0 = (tile % a.mtiles) * BT, n0 = (tile / a.mtiles) * BT;
  const int s0 = sl * a.per, s1 = min(s0 + a.per, a.steps);

  // the loader's rows (64 apart) and piece; a row past filters is marked, a
  // row past K reads the table's sentinels (outside every window)
  const int lr = tid >> 2, q = tid & 3;
  int frow[T], boff[T], bwin[T];
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const int f = m0 + j * 64 + lr, n = n0 + j * 64 + lr;
    frow[j] = f < a.filters ? f * a.ohw : -1;
    boff[j] = a.ktab[n] >> 2;
    bwin[j] = a.ktab[a.ktab_n + n];
  }
  unsigned char* const wrow = &lds[0][0][0] + lr * kRow + q * 16;
  const unsigned char* const ra = &lds[0][0][0] + (wm * 32 * T + lc) * kRow + h * 16;
  const unsigned char* const rb = &lds[0][1][0] + (wn * 32 * T + lc) * kRow + h * 16;

  f32x16 acc[T][T];
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  float ga[T][8], gb[T][8];
  gather_dw<T>(a, s0, q, frow, boff, bwin, ga, gb);
#pragma unroll
  for (int j = 0; j < T; ++j) {
    store_b<8>(wrow + j * 64 * kRow, ga[j]);
    store_b<8>(wrow + kBuf + j * 64 * kRow, gb[j]);
  }
  __syncthreads();

  for (int s = s0; s < s1; ++s) {
    const bool more = s + 1 < s1;
    if (more) gather_dw<T>(a, s + 1, q, frow, boff, bwin, ga, gb);
    const int cur = ((s - s0) & 1) * 2 * kBuf;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      bf16x8 af[T], bf[T];
#pragma unroll
      for (int i = 0; i < T; ++i) {
        af[i] = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const uint4*>(ra + cur + i * 32 * kRow + hh * 32));
        bf[i] = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const uint4*>(rb + cur + i * 32 * kRow + hh * 32));
      }
#pragma unroll
      for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
          acc[i][j] =
              __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      const int nxt = ((s + 1 - s0) & 1) * 2 * kBuf;
#pragma unroll
      for (int j = 0; j < T; ++j) {
        store_b<8>(wrow + nxt + j * 64 * kRow, ga[j]);
        store_b<8>(wrow + nxt + kBuf + j * 64 * kRow, gb[j]);
      }
    }
    __syncthreads();
  }

  // epilogue: lane l holds column n = l % 32 and rows 8*(e/4) + 4*(l/32) + e%4
  float* const o = a.out + (a.partial ? (int64_t)sl * a.filters * a.K : 0);
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const int n = n0 + wn * 32 * T + j * 32 + lc;
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const int f0 = m0 + wm * 32 * T + i * 32 + 4 * h;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int f = f0 + (e & 3) + 8 * (e >> 2);
        if (f < a.filters && n < a.K) {
          float* const w = o + (int64_t)f * a.K + n;
          *w = a.partial ? acc[i][j][e] : *w + acc[i][j][e];
        }
      }
    }
  }
}

// weight_updates += part[0] + part[1] + ... + part[S-1], in that order
__global__ void __launch_bounds__(kThreads)
conv_bf16_dw_sum_kernel(int64_t n, int S, const float* __restrict__ part,
                        float* __restrict__ wu) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float t = part[i];
  for (int s = 1; s < S; ++s) t += part[s * n + i];
  wu[i] += t;
}

}  // namespace

hipError_t launch_conv_bf16_dx(int tile, const ConvBf16BwdArgs& c, hipStream_t s) {
  const int64_t kk = c.ks * c.ks, Kd = c.filters * kk;
  const int bm = tile == 0 ? 128 : 64, bn = bm;
  const int64_t pieces = conv_bf16_packed_bytes(c.C, Kd) / 16;
  const int64_t pblocks = (pieces + kThreads - 1) / kThreads;
  DxArgs a{};
  a.delta = c.delta;
  a.packed = reinterpret_cast<const uint4*>(c.packed_wt);
  a.sd = c.state_delta;
  a.ktab = c.ktab_delta;
  a.ktab_n = (int)(Kd + KTAB_PAD);
  a.N = c.batch * c.H * c.W;
  a.dimg = c.filters * c.oh * c.ow;
  a.simg = c.C * c.H * c.W;
  a.W = (int)c.W, a.HW = (int)(c.H * c.W), a.oh = (int)c.oh, a.ow = (int)c.ow;
  a.stride = (int)c.stride, a.pad = (int)c.pad, a.C = (int)c.C;
  a.sshift = c.stride == 1 ? 0 : c.stride == 2 ? 1 : -1;
  a.steps = (int)((Kd + kStep - 1) / kStep);
  a.ks16 = 2 * a.steps;
  a.mtiles = (int)((c.C + bm - 1) / bm);
  const int64_t blocks = a.mtiles * ((a.N + bn - 1) / bn);
  if (tile < 0 || tile >= conv_bf16_tile_count() || blocks > 0x7fffffffLL ||
      pblocks > 0x7fffffffLL)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(conv_bf16_pack_wt_kernel, dim3((unsigned)pblocks), dim3(kThreads), 0, s,
                     pieces, (int)c.C, (int)c.filters, (int)kk, a.ks16, c.weights,
                     reinterpret_cast<uint4*>(c.packed_wt));
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  const dim3 grid((unsigned)blocks), block(kThreads);
  if (tile == 0)
    hipLaunchKernelGGL((conv_bf16_dx_kernel<2, 2>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((conv_bf16_dx_kernel<1, 1>), grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_conv_bf16_dw(int split, const ConvBf16BwdArgs& c, hipStream_t s) {
  const int64_t K = c.C * c.ks * c.ks, R = c.batch * c.oh * c.ow;
  const int bt = conv_bf16_dw_tile(c.filters, K) == 0 ? 128 : 64;
  Bf16DwArgs a{};
  a.delta = c.delta;
  a.in = c.input;
  a.ktab = c.ktab_in;
  a.ktab_n = (int)(K + KTAB_PAD);
  a.chw = c.C * c.H * c.W;
  a.dimg = c.filters * c.oh * c.ow;
  a.R = (int)R, a.ohw = (int)(c.oh * c.ow), a.oh = (int)c.oh, a.ow = (int)c.ow;
  a.H = (int)c.H, a.W = (int)c.W, a.stride = (int)c.stride, a.pad = (int)c.pad;
  a.filters = (int)c.filters, a.K = (int)K;
  a.steps = (int)((R + kStep - 1) / kStep);
  // (the slices as the planner leaves them: none is empty)
  split = std::max(1, std::min(split, a.steps));
  a.per = (a.steps + split - 1) / split;
  split = (a.steps + a.per - 1) / a.per;
  a.mtiles = (int)((c.filters + bt - 1) / bt);
  a.ntiles = (int)((K + bt - 1) / bt);
  a.partial = split > 1;
  a.out = a.partial ? c.dw_part : c.weight_updates;
  const int64_t blocks = (int64_t)a.mtiles * a.ntiles * split;
  if (blocks > 0x7fffffffLL || (a.partial && !c.dw_part)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kThreads);
  if (bt == 128)
    hipLaunchKernelGGL((conv_bf16_dw_kernel<2>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((conv_bf16_dw_kernel<1>), grid, block, 0, s, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess || !a.partial) return e;
  const int64_t n = c.filters * K;
  hipLaunchKernelGGL(conv_bf16_dw_sum_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, n, split, c.dw_part, c.weight_updates);
  return hipGetLastError();
}

}  // namespace tns

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
