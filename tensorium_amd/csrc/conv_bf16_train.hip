// conv_bf16_train.hip — convolution forward on the bf16 MFMA from the plain fp32
// weights, the training forward of the opt-in reduced-precision path
// ("bf16 conv training forward").  The implicit GEMM, the B side,
// the accumulators and the tiles are conv_bf16.hip's: M = filters, N = batch *
// oh * ow, K = C * k * k in (c, ky, kx) order, steps of kStep = 32 = two MFMAs
// of depth 16, 2 x 2 waves on 128 x 128 (form 0) or 64 x 64 (form 1).  What
// differs is A: in training the weights change every step, so nothing is
// packed; the kernel takes the row-major fp32 [filters][K] matrix that update
// wrote and rounds it on its way in.
//
//   A (weights)  a step's tile is BM rows x 32 k of fp32.  A thread takes four
//                consecutive k of a row: eight consecutive lanes read the 128
//                bytes of one row's step (one 16-byte load each where the
//                matrix is 16-byte aligned and K a multiple of 4, else four
//                4-byte loads), the wave's eight lane groups take rows 4
//                apart, the four waves rows 0..3 of those, so that a pass of
//                the block covers 32 rows:
//                    row = 32 * pass + 4 * (lane / 8) + wave,  k = 4 * (lane % 8).
//                Rows at or beyond filters and k at or beyond K read element 0
//                of the matrix and are replaced by zeros: nothing is read
//                outside it.  The four floats become two bf16 pairs
//                (v_cvt_pk_bf16_f32: nearest even, Inf and NaN kept) and go to
//                LDS as one 8-byte store at row * kRow + 8 * (lane % 8), rows
//                k-contiguous like B's.
//                Banks, with kRow = 80 bytes = 20 dwords.  The fragment read
//                is B's (lane l: row l%32, the 16-byte piece l/32 of the
//                MFMA's half): eight consecutive rows' pieces start at dwords
//                20 r mod 32 = 0, 20, 8, 28, 16, 4, 24, 12, every bank once
//                (and sixteen rows 20 r mod 64, every multiple of 4 once,
//                where the LDS has 64 banks).  The store: a row's eight
//                lanes write 16 consecutive dwords, and the next lane group's
//                row is 4 further, 4 * 20 = 80 = 16 mod 32 dwords on: sixteen
//                consecutive lanes (two rows) cover the 32 banks once, and
//                thirty-two lanes (rows r, r+4, r+8, r+12 at dwords 0, 16,
//                32, 48 mod 64) cover 64 banks once.  That is why the lane
//                groups take rows 4 apart and not consecutive ones: rows r and
//                r+1 would meet in banks 20..31 mod 32.
//   B (pixels)   conv_bf16.hip's: the k-table gather from the unpadded fp32
//                images, rounded in registers, 16-byte stores into rows of kRow.
//   LDS          a buffer holds B's BN rows and then A's BM rows, (BN + BM) * 80
//                bytes; two buffers.  The loads of step i+1 (A and B) are
//                issued before the MFMAs of step i and stored behind them into
//                the other buffer, whose last readers passed the barrier that
//                ended step i-1: one barrier a step.  128 x 128: 40960 bytes a
//                block, three blocks a CU (the occupancy conv_bf16.hip's
//                kernel has, by registers) in 122880 of 163840 bytes.
//   C            conv_bf16.hip's accumulators.  EPI 0 stores them raw (the
//                batch-norm layers' x, before any bias), EPI 1 / 2 add the
//                bias and apply the activation (2: exp in double).  No
//                atomics, no split k: the same call gives the same bits.
//
// The A fragment a lane reads holds the same k in the same register slots as
// conv_bf16.hip's packed one, so a tile sums the same exact products in the
// same MFMA order: for the same tile the result is conv_bf16.hip's bit for bit.
#include "tns_internal.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "conv_bf16_common.hpp"
#include "tns_act.hpp"

namespace tns {
namespace {

using namespace bf16k;

struct TrainArgs {
  const float* in;
  const float* w;
  const float* bias;
  float* out;
  const int* ktab;
  int64_t N, chw, out_img;  // columns; floats an input image; floats an output image
  int ktab_n, H, W, ow, ohw, stride, pad, filters, act;
  int K, steps, mtiles;  // C*k*k; K / 32 rounded up; tiles over the filters
};

struct Column {
  const float* img;
  int pix, iy0, ix0;
};

// KPT consecutive k of step s for the thread's column (conv_bf16.hip's gather)
template <int KPT>
__device__ __forceinline__ void gather(const TrainArgs& a, const Column& c, int k0,
                                       float (&g)[KPT]) {
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const int off = a.ktab[k0 + i], win = a.ktab[a.ktab_n + k0 + i];
    const int iy = c.iy0 + (win & 0xffff), ix = c.ix0 + (win >> 16);
    const bool ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
    const float x = c.img[ok ? c.pix + (off >> 2) : 0];
    g[i] = ok ? x : 0.0f;
  }
}

// The thread's four k (k0 .. k0+3) of its row in each of the AP passes.  p0:
// the start of its row of pass 0 (formed, never read, where the row is outside
// the matrix); row0: that row
template <int AP, bool VEC>
__device__ __forceinline__ void load_a(const TrainArgs& a, const float* p0, int row0, int k0,
                                       float4 (&r)[AP]) {
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const bool rok = row0 + 32 * i < a.filters;
    const float* const p = p0 + (int64_t)(32 * i) * a.K + k0;
    if (VEC) {  // K % 4 == 0: the piece is inside the row or behind it
      const bool ok = rok && k0 < a.K;
      const float4 v = *reinterpret_cast<const float4*>(ok ? p : a.w);
      r[i] = ok ? v : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = rok && k0 + j < a.K;
        const float x = *(ok ? p + j : a.w);
        v[j] = ok ? x : 0.0f;
      }
      r[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// ... rounded, one 8-byte store a pass (dst: the thread's place in pass 0)
template <int AP>
__device__ __forceinline__ void store_a(unsigned char* dst, const float4 (&r)[AP]) {
#pragma unroll
  for (int i = 0; i < AP; ++i)
    *reinterpret_cast<uint2*>(dst + i * 32 * kRow) =
        make_uint2(bf16_pair(r[i].x, r[i].y), bf16_pair(r[i].z, r[i].w));
}

// grid: mtiles * column tiles, the filter tiles of one column tile side by side
template <int TM, int TN, int EPI, bool VEC>
__global__ void __launch_bounds__(kThreads) conv_bf16_train_kernel(const TrainArgs a) {
  constexpr int BM = 64 * TM, BN = 64 * TN, KPT = BN / 8, AP = BM / 32;
  constexpr int kBuf = (BN + BM) * kRow;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][kBuf];
  const int tid = threadIdx.x, lane = tid & 63, lc = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int mt = blockIdx.x % a.mtiles;
  const int64_t n0 = (int64_t)(blockIdx.x / a.mtiles) * BN;

  // B: the gather's column and k range
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

  // A: the thread's row of pass 0 and its four k of a step
  const int arl = 4 * (lane >> 3) + wave, ak = 4 * (lane & 7);
  const int arow = mt * BM + arl;
  const float* const ap = a.w + (int64_t)arow * a.K;
  unsigned char* const awrow = &lds[0][0] + (BN + arl) * kRow + ak * 2;

  // where the wave's fragments lie in a buffer
  const unsigned char* const rrow = &lds[0][0] + (wn * 32 * TN + lc) * kRow + h * 16;
  const unsigned char* const arrow = &lds[0][0] + (BN + wm * 32 * TM + lc) * kRow + h * 16;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  float g[KPT];
  float4 ar[AP];
  gather<KPT>(a, col, gk, g);
  load_a<AP, VEC>(a, ap, arow, ak, ar);
  store_b<KPT>(wrow, g);
  store_a<AP>(awrow, ar);
  __syncthreads();

  for (int s = 0; s < a.steps; ++s) {
    const bool more = s + 1 < a.steps;
    if (more) {
      gather<KPT>(a, col, (s + 1) * kStep + gk, g);
      load_a<AP, VEC>(a, ap, arow, (s + 1) * kStep + ak, ar);
    }
    const int cur = (s & 1) * kBuf;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      bf16x8 af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        af[i] = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const uint4*>(arrow + cur + i * 32 * kRow + hh * 32));
#pragma unroll
      for (int j = 0; j < TN; ++j)
        bf[j] = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const uint4*>(rrow + cur + j * 32 * kRow + hh * 32));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      const int nxt = ((s + 1) & 1) * kBuf;
      store_b<KPT>(wrow + nxt, g);
      store_a<AP>(awrow + nxt, ar);
    }
    __syncthreads();
  }

  // epilogue: raw, or bias and activation; fp32 stores (32 consecutive columns a row)
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
          if (EPI == 0) {
            o[(int64_t)f * a.ohw] = acc[i][j][e];
          } else {
            const float v = acc[i][j][e] + a.bias[f];
            o[(int64_t)f * a.ohw] = EPI == 2 ? act_apply(v, a.act) : act_apply_cheap(v, a.act);
          }
        }
      }
    }
  }
}

template <int TM, int TN, int EPI>
void launch(bool vec, dim3 grid, hipStream_t s, const TrainArgs& a) {
  if (vec)
    hipLaunchKernelGGL((conv_bf16_train_kernel<TM, TN, EPI, true>), grid, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((conv_bf16_train_kernel<TM, TN, EPI, false>), grid, dim3(kThreads), 0, s, a);
}

template <int TM, int TN>
void launch(int epi, bool vec, dim3 grid, hipStream_t s, const TrainArgs& a) {
  if (epi == 0) launch<TM, TN, 0>(vec, grid, s, a);
  else if (epi == 1) launch<TM, TN, 1>(vec, grid, s, a);
  else launch<TM, TN, 2>(vec, grid, s, a);
}

}  // namespace

hipError_t launch_conv_bf16_weights(int tile, const ConvBf16Args& c, const float* weights,
                                    hipStream_t s) {
  const int64_t K = c.C * c.ks * c.ks;
  const int bm = tile == 0 ? 128 : 64, bn = bm;
  TrainArgs a{};
  a.in = c.input;
  a.w = weights;
  a.bias = c.bias;
  a.out = c.out;
  a.ktab = c.ktab;
  a.ktab_n = (int)(K + KTAB_PAD);
  a.N = c.batch * c.oh * c.ow;
  a.chw = c.C * c.H * c.W;
  a.out_img = c.filters * c.oh * c.ow;
  a.H = (int)c.H, a.W = (int)c.W, a.ow = (int)c.ow, a.ohw = (int)(c.oh * c.ow);
  a.stride = (int)c.stride, a.pad = (int)c.pad, a.filters = (int)c.filters, a.act = c.act;
  a.K = (int)K;
  a.steps = (int)((K + kStep - 1) / kStep);
  a.mtiles = (int)((c.filters + bm - 1) / bm);
  const int64_t blocks = a.mtiles * ((a.N + bn - 1) / bn);
  if (tile < 0 || tile >= conv_bf16_tile_count() || blocks > 0x7fffffffLL)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks);
  // 16-byte loads where every row starts on a 16-byte boundary
  const bool vec = K % 4 == 0 && (reinterpret_cast<uintptr_t>(weights) & 15) == 0;
  const int epi = !c.bias ? 0 : act_transcendental(c.act) ? 2 : 1;
  if (tile == 0) launch<2, 2>(epi, vec, grid, s, a);
  else launch<1, 1>(epi, vec, grid, s, a);
  return hipGetLastError();
}

}  // namespace tns

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
