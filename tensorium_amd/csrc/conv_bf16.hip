// conv_bf16.hip — convolution forward on the bf16 MFMA (v_mfma_f32_32x32x16_bf16),
// the opt-in reduced-precision inference path ("bf16 conv forward").
// Operands are rounded to bf16 (nearest even); products are exact in fp32 and
// accumulated in fp32; bias, activation and the stored output are fp32.  No
// claim of bit parity with the fp32 paths: the accumulation order inside a
// tile is the MFMA's and differs between the tile shapes.
//
// One implicit GEMM: M = filters, N = batch * oh * ow (the batch folded into
// the columns), K = C * k * k in the library's (c, ky, kx) order, run in steps
// of kStep = 32 = two MFMAs of depth 16.
//
//   A (weights)  packed once by conv_bf16_pack_kernel: rows padded to kPackRows,
//                K to a multiple of kStep with zeros.  For the 32-row block mb
//                and the depth-16 step ks, lane l's fragment (row mb*32 + l%32,
//                k = ks*16 + 8*(l/32) .. +7) is the 16-byte piece
//                ((mb * K/16 + ks) * 64 + l): a wave's fragment for one MFMA
//                is one contiguous KiB, read straight into registers (the
//                weights stay in L2 across a layer's column tiles), one step
//                ahead of the MFMAs that use it.
//   B (pixels)   gathered from the unpadded fp32 images through the k-table
//                (get_ktab: plane offset and tap displacement per k, sentinels
//                behind K), the window bounds checked, zeros outside.  A thread
//                owns one pixel column of the tile and KPT consecutive k of the
//                step: for one k the lanes of a wave read consecutive pixels,
//                and the table entries are wave-uniform (scalar loads).  The
//                floats become bf16 pairs in registers (v_cvt_pk_bf16_f32) and
//                go to LDS k-contiguous per pixel, 64 bytes of data in a row
//                of kRow = 80: with that stride eight consecutive rows' 16-byte
//                pieces cover every bank once, for the writes and for the
//                fragment reads (lane l: row l%32, piece (l/32) of the MFMA's
//                half).  Two LDS buffers: the loads of step i+1 are issued
//                before the MFMAs of step i and written behind them; one
//                barrier a step.
//   C            fp32 accumulators, TM x TN MFMA tiles a wave, 2 x 2 waves a
//                block: 128 x 128 (form 0) for the large planes, 64 x 64
//                (form 1) where the large tile would leave CUs idle.  Lane l
//                holds column l%32 and rows 8*(e/4) + 4*(l/32) + e%4 of each
//                32 x 32 tile; the epilogue adds the bias, applies the
//                activation and stores.  No atomics, no split k: the same call
//                gives the same bits.
//
// Only the i / j mapping of the MFMA matters here: A and B fragments assign
// the same k to the same register slot, so any order of the 16 k inside the
// instruction gives the same sum of exact products.
#include "tns_internal.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "conv_bf16_common.hpp"
#include "tns_act.hpp"

namespace tns {
namespace {

using namespace bf16k;

struct Bf16Args {
  const float* in;
  const uint4* packed;
  const float* bias;
  float* out;
  const int* ktab;
  int64_t N, chw, out_img;  // columns; floats an input image; floats an output image
  int ktab_n, H, W, ow, ohw, stride, pad, filters, act;
  int steps, ks16, mtiles;  // K / 32, K / 16 (padded K), tiles over the filters
};

// one thread per 16-byte piece of the packed buffer
__global__ void __launch_bounds__(kThreads)
conv_bf16_pack_kernel(int64_t pieces, int filters, int K, int ks16, const float* __restrict__ w,
                      uint4* __restrict__ packed) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= pieces) return;
  const int lane = (int)(q & 63);
  const int64_t frag = q >> 6;
  const int ks = (int)(frag % ks16);
  const int64_t row = (frag / ks16) * 32 + (lane & 31);
  const int k0 = ks * 16 + 8 * (lane >> 5);
  unsigned v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    v[i] = (row < filters && k0 + i < K) ? bf16_rne(w[row * K + k0 + i]) : 0u;
  packed[q] = make_uint4(v[0] | v[1] << 16, v[2] | v[3] << 16, v[4] | v[5] << 16,
                         v[6] | v[7] << 16);
}

// what a thread needs to gather its pixel column: the image, the window's
// first element relative to it, and the window's first row / column (a column
// past N: a row no tap brings inside the image)
struct Column {
  const float* img;
  int pix, iy0, ix0;
};

// KPT consecutive k of step s for the thread's column.  Every load is inside
// the image: an outside tap reads element 0 and is replaced by zero
template <int KPT>
__device__ __forceinline__ void gather(const Bf16Args& a, const Column& c, int k0, float (&g)[KPT]) {
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const int off = a.ktab[k0 + i], win = a.ktab[a.ktab_n + k0 + i];
    const int iy = c.iy0 + (win & 0xffff), ix = c.ix0 + (win >> 16);
    const bool ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
    const float x = c.img[ok ? c.pix + (off >> 2) : 0];
    g[i] = ok ? x : 0.0f;
  }
}

// grid: mtiles * column tiles, the filter tiles of one column tile side by
// side (they gather the same pixels).  EXP: the logistic / tanh epilogue (exp
// in double), kept out of the other activations' instantiation
template <int TM, int TN, bool EXP>
__global__ void __launch_bounds__(kThreads) conv_bf16_kernel(const Bf16Args a) {
  constexpr int BN = 64 * TN, KPT = BN / 8;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][BN * kRow];
  const int tid = threadIdx.x, lane = tid & 63, lc = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int mt = blockIdx.x % a.mtiles;
  const int64_t n0 = (int64_t)(blockIdx.x / a.mtiles) * BN;

  // the gather's column and k range
  const int gp = tid % BN;
  const int gk = __builtin_amdgcn_readfirstlane(tid / BN) * KPT;
  Column col{a.in, 0, -0x8000, 0};
  if (n0 + gp < a.N) {
    const int64_t b = (n0 + gp) / a.ohw;
    const int p = (int)(n0 + gp - b * a.ohw);
    const int oy = p / a.ow, ox = p - oy * a.ow;
    col.iy0 = oy * a.stride - a.pad;
    col.ix0 = ox * a.stride - a.pad;
    col.img = a.in + b * a.chw;
    col.pix = col.iy0 * a.W + col.ix0;
  }
  unsigned char* const wrow = &lds[0][0] + gp * kRow + gk * 2;

  // the wave's A fragments: 32-row block mt * 2TM + wm * TM + i
  const uint4* ap[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
    ap[i] = a.packed + (int64_t)(mt * 2 * TM + wm * TM + i) * a.ks16 * 64 + lane;
  // ... and where its B fragments lie in a buffer
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
  gather<KPT>(a, col, gk, g);
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
      gather<KPT>(a, col, (s + 1) * kStep + gk, g);
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

  // epilogue: bias, activation, fp32 stores (32 consecutive columns a row)
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int64_t n = n0 + wn * 32 * TN + j * 32 + lc;
    const bool inside = n < a.N;
    const int64_t b = inside ? n / a.ohw : 0;
    float* const o = a.out + b * a.out_img + (n - b * a.ohw);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int f0 = (mt * 2 * TM + wm * TM + i) * 32 + 4 * h;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int f = f0 + (e & 3) + 8 * (e >> 2);
        if (inside && f < a.filters) {
          const float v = acc[i][j][e] + a.bias[f];
          o[(int64_t)f * a.ohw] = EXP ? act_apply(v, a.act) : act_apply_cheap(v, a.act);
        }
      }
    }
  }
}

}  // namespace

int conv_bf16_tile_count() { return 2; }

const char* conv_bf16_tile_name(int v) {
  return v == 0 ? "bf16_128x128" : v == 1 ? "bf16_64x64" : "";
}

int64_t conv_bf16_packed_bytes(int64_t filters, int64_t K) {
  const int64_t rows = (filters + kPackRows - 1) / kPackRows * kPackRows;
  const int64_t kp = (K + kStep - 1) / kStep * kStep;
  return rows * kp * 2;
}

hipError_t launch_conv_bf16_pack(int64_t filters, int64_t K, const float* weights, void* packed,
                                 hipStream_t s) {
  const int64_t pieces = conv_bf16_packed_bytes(filters, K) / 16;
  const int64_t blocks = (pieces + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffLL || K > 0x7fffffffLL || filters > 0x7fffffffLL)
    return hipErrorInvalidValue;
  const int ks16 = (int)((K + kStep - 1) / kStep * 2);
  hipLaunchKernelGGL(conv_bf16_pack_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, pieces,
                     (int)filters, (int)K, ks16, weights, reinterpret_cast<uint4*>(packed));
  return hipGetLastError();
}

hipError_t launch_conv_bf16(int tile, const ConvBf16Args& c, hipStream_t s) {
  const int64_t K = c.C * c.ks * c.ks;
  const int bm = tile == 0 ? 128 : 64, bn = bm;
  Bf16Args a{};
  a.in = c.input;
  a.packed = reinterpret_cast<const uint4*>(c.packed);
  a.bias = c.bias;
  a.out = c.out;
  a.ktab = c.ktab;
  a.ktab_n = (int)(K + KTAB_PAD);
  a.N = c.batch * c.oh * c.ow;
  a.chw = c.C * c.H * c.W;
  a.out_img = c.filters * c.oh * c.ow;
  a.H = (int)c.H, a.W = (int)c.W, a.ow = (int)c.ow, a.ohw = (int)(c.oh * c.ow);
  a.stride = (int)c.stride, a.pad = (int)c.pad, a.filters = (int)c.filters, a.act = c.act;
  a.steps = (int)((K + kStep - 1) / kStep);
  a.ks16 = 2 * a.steps;
  a.mtiles = (int)((c.filters + bm - 1) / bm);
  const int64_t blocks = a.mtiles * ((a.N + bn - 1) / bn);
  if (tile < 0 || tile >= conv_bf16_tile_count() || blocks > 0x7fffffffLL)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(kThreads);
  const bool ex = act_transcendental(c.act);
  if (tile == 0 && ex)
    hipLaunchKernelGGL((conv_bf16_kernel<2, 2, true>), grid, block, 0, s, a);
  else if (tile == 0)
    hipLaunchKernelGGL((conv_bf16_kernel<2, 2, false>), grid, block, 0, s, a);
  else if (ex)
    hipLaunchKernelGGL((conv_bf16_kernel<1, 1, true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((conv_bf16_kernel<1, 1, false>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace tns

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
