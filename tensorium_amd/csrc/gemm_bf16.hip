// gemm_bf16.hip — the row-major product C[M][N] = op(A) . op(B) (+ C) on the
// bf16 MFMA, the opt-in reduced-precision path of the connected, lstm and rnn
// layers ("bf16 GEMM").  A and B are fp32 in global memory and are
// rounded to bf16 (nearest even) on their way into LDS; products are exact in
// fp32, accumulated in fp32 and stored (or added to C) in fp32.  No atomics: the
// same call gives the same bits.  No claim of bit parity with the fp32 SGEMM:
// the accumulation order is the MFMA's and differs between tiles and slice
// counts.
//
// LDS  Both operands lie k-contiguous per row, kStep = 32 k (64 bytes) in a row
//      of kRow = 80, the convolution kernels' geometry (conv_bf16_common.hpp):
//      with that stride eight consecutive rows' 16-byte pieces cover every bank
//      once, for the writes and for the fragment reads.  Two stages of
//      [A rows | B rows]; the loads of step i + 1 are issued before the MFMAs of
//      step i and written behind them; one barrier a step.
//
// Loaders, one per place k can lie in memory (a form pairs two of them):
//   kc  k contiguous (NT's A and B, NN's A).  A thread owns one 16-byte LDS
//       piece: row idx / 4, k = 8 * (idx % 4) .. + 7; it reads two float4 where
//       the operand's base and leading dimension are multiples of 16 bytes and
//       the piece lies inside K, else eight guarded floats (the callers pass
//       float offsets into slabs), rounds them in registers
//       (v_cvt_pk_bf16_f32) and writes the piece.
//   ks  k slow (TN's A and B, NN's B): element (row, k) is P[k * ld + row].  A
//       thread owns row idx % ROWS and the 8 k of piece idx / ROWS: for one k
//       the lanes of a wave read consecutive floats (coalesced along m or n);
//       the eight values a thread gathered are one row's k-contiguous piece, so
//       the transposition is the LDS write and the fragment reads stay 16-byte.
//   pk  B packed once by gemm_bf16_pack_kernel ([N][Kp] bf16, Kp = K rounded up
//       to kStep with zeros): the thread of the kc mapping copies one 16-byte
//       piece, always aligned, with no rounding and half the bytes.
//
// Tiles (4 waves a block):
//   0  64 x 64, v_mfma_f32_32x32x16_bf16: 2 x 2 waves of one 32 x 32 tile; lane
//      l reads row l % 32, k = 16 * hh + 8 * (l / 32) .. + 7 of both operands
//      for the step's MFMA hh and holds column l % 32, rows 8 * (e / 4) +
//      4 * (l / 32) + e % 4.
//   1  16 x 128, v_mfma_f32_16x16x32_bf16, where M <= 16 makes the 32-row tile
//      mostly padding (the batch-1 inference row, a few streams): a wave holds
//      two 16 x 16 tiles side by side; lane l reads row l % 16, k = 8 * (l / 16)
//      .. + 7 (one MFMA a step) and holds column l % 16, rows 4 * (l / 16) + e.
//   A and B fragments assign the same k to the same register slot, so any order
//   of the k inside the instruction gives the same sum of exact products.
//
// Slices  Few rows times a few hundred columns are a handful of tiles on 256
//   CUs: the reduction is cut into S contiguous slices of steps
//   (gemm_bf16_split); slice sl of a tile writes its fp32 partial to scratch
//   [S][M][N], and gemm_bf16_sum_kernel adds the slices in the order 0 .. S-1
//   and then C's prior value (accumulate).  With S = 1 the main kernel stores
//   or adds into C itself.
#include <algorithm>

#include "tns_internal.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "conv_bf16_common.hpp"

namespace tns {
namespace {

using namespace bf16k;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Bf16GemmArgs {
  const float* A;
  const float* B;       // fp32, or the packed bf16 matrix (form NTP)
  float* out;           // C, or the partials [S][M][N]
  int64_t lda, ldb, ldo;
  int M, N, K;
  int steps, per, mtiles, ntiles;  // reduction steps of 32; steps a slice
  int partial, accumulate, va, vb;  // va / vb: 16-byte loads of a kc operand
};

// ---- loaders: NP pieces a thread, piece idx = tid + 256 * p of the ROWS * 4 ----
template <int ROWS>
struct Pieces {
  static constexpr int NP = ROWS * 4 >= kThreads ? ROWS * 4 / kThreads : 1;
  float g[NP][8];
};

template <int ROWS>
__device__ __forceinline__ void load_kc(const float* __restrict__ P, int64_t ld, int row0,
                                        int nrows, int k0, int K, bool vec, int tid,
                                        Pieces<ROWS>& r) {
#pragma unroll
  for (int p = 0; p < Pieces<ROWS>::NP; ++p) {
    const int idx = tid + kThreads * p;
    const int row = row0 + (idx >> 2), k = k0 + 8 * (idx & 3);
    const bool in = idx < ROWS * 4 && row < nrows;
    const float* const src = P + (int64_t)(in ? row : 0) * ld + k;
    if (in && vec && k + 8 <= K) {
      const float4 x = reinterpret_cast<const float4*>(src)[0];
      const float4 y = reinterpret_cast<const float4*>(src)[1];
      r.g[p][0] = x.x, r.g[p][1] = x.y, r.g[p][2] = x.z, r.g[p][3] = x.w;
      r.g[p][4] = y.x, r.g[p][5] = y.y, r.g[p][6] = y.z, r.g[p][7] = y.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) r.g[p][e] = (in && k + e < K) ? src[e] : 0.0f;
    }
  }
}

template <int ROWS>
__device__ __forceinline__ void load_ks(const float* __restrict__ P, int64_t ld, int row0,
                                        int nrows, int k0, int K, int tid, Pieces<ROWS>& r) {
#pragma unroll
  for (int p = 0; p < Pieces<ROWS>::NP; ++p) {
    const int idx = tid + kThreads * p;
    const int row = row0 + idx % ROWS, k = k0 + 8 * (idx / ROWS);
    const bool in = idx < ROWS * 4 && row < nrows;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      r.g[p][e] = (in && k + e < K) ? P[(int64_t)(k + e) * ld + row] : 0.0f;
  }
}

// the packed matrix: row stride Kp = steps * kStep bf16, pieces of 8
template <int ROWS>
__device__ __forceinline__ void load_pk(const uint4* __restrict__ P, int64_t pieces_row, int row0,
                                        int nrows, int s, int tid, uint4 (&v)[Pieces<ROWS>::NP]) {
#pragma unroll
  for (int p = 0; p < Pieces<ROWS>::NP; ++p) {
    const int idx = tid + kThreads * p;
    const int row = row0 + (idx >> 2);
    const bool in = idx < ROWS * 4 && row < nrows;
    v[p] = in ? P[(int64_t)row * pieces_row + 4 * s + (idx & 3)] : make_uint4(0, 0, 0, 0);
  }
}

// piece idx of a kc / pk operand is (row idx / 4, piece idx % 4), of a ks
// operand (row idx % ROWS, piece idx / ROWS)
template <int ROWS, bool KS>
__device__ __forceinline__ unsigned char* piece_at(unsigned char* buf, int idx) {
  return KS ? buf + (idx % ROWS) * kRow + (idx / ROWS) * 16 : buf + (idx >> 2) * kRow + (idx & 3) * 16;
}

template <int ROWS, bool KS>
__device__ __forceinline__ void store_pieces(unsigned char* buf, int tid, const Pieces<ROWS>& r) {
#pragma unroll
  for (int p = 0; p < Pieces<ROWS>::NP; ++p) {
    const int idx = tid + kThreads * p;
    if (idx < ROWS * 4) store_b<8>(piece_at<ROWS, KS>(buf, idx), r.g[p]);
  }
}

enum { FORM_NT = 0, FORM_TN = 1, FORM_NN = 2, FORM_NTP = 3 };

// grid: tiles * slices, the row tiles of one column tile side by side (they
// read the same B rows).  TILE 0: 64 x 64; TILE 1: 16 x 128
template <int FORM, int TILE>
__global__ void __launch_bounds__(kThreads) gemm_bf16_kernel(const Bf16GemmArgs a) {
  constexpr int BM = TILE == 0 ? 64 : 16, BN = TILE == 0 ? 64 : 128;
  constexpr bool AKS = FORM == FORM_TN, BKS = FORM == FORM_TN || FORM == FORM_NN;
  constexpr bool BPK = FORM == FORM_NTP;
  constexpr int kStage = (BM + BN) * kRow;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][kStage];  // [stage][A | B]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles = a.mtiles * a.ntiles;
  const int tile = blockIdx.x % tiles, sl = blockIdx.x / tiles;
  const int m0 = (tile % a.mtiles) * BM, n0 = (tile / a.mtiles) * BN;
  const int s0 = sl * a.per, s1 = min(s0 + a.per, a.steps);
  const uint4* const packed = reinterpret_cast<const uint4*>(a.B);

  Pieces<BM> ra;
  Pieces<BN> rb;
  uint4 vb[Pieces<BN>::NP];
  auto load = [&](int s) {
    const int k0 = s * kStep;
    if constexpr (AKS)
      load_ks<BM>(a.A, a.lda, m0, a.M, k0, a.K, tid, ra);
    else
      load_kc<BM>(a.A, a.lda, m0, a.M, k0, a.K, a.va, tid, ra);
    if constexpr (BPK)
      load_pk<BN>(packed, 4 * (int64_t)a.steps, n0, a.N, s, tid, vb);
    else if constexpr (BKS)
      load_ks<BN>(a.B, a.ldb, n0, a.N, k0, a.K, tid, rb);
    else
      load_kc<BN>(a.B, a.ldb, n0, a.N, k0, a.K, a.vb, tid, rb);
  };
  auto store = [&](unsigned char* stage) {
    store_pieces<BM, AKS>(stage, tid, ra);
    if constexpr (BPK) {
#pragma unroll
      for (int p = 0; p < Pieces<BN>::NP; ++p)
        *reinterpret_cast<uint4*>(piece_at<BN, false>(stage + BM * kRow, tid + kThreads * p)) = vb[p];
    } else {
      store_pieces<BN, BKS>(stage + BM * kRow, tid, rb);
    }
  };

  // the wave's fragment rows in a stage, and its accumulators
  constexpr int NACC = TILE == 0 ? 16 : 8;  // one 32 x 32 tile, or two 16 x 16
  float acc[NACC];
#pragma unroll
  for (int e = 0; e < NACC; ++e) acc[e] = 0.0f;
  const int lc = TILE == 0 ? lane & 31 : lane & 15, h = TILE == 0 ? lane >> 5 : lane >> 4;
  const int wm = TILE == 0 ? wave & 1 : 0, wn = TILE == 0 ? wave >> 1 : wave;
  const unsigned char* const fa = &lds[0][0] + (wm * 32 + lc) * kRow + h * 16;
  const unsigned char* const fb = &lds[0][0] + (BM + wn * 32 + lc) * kRow + h * 16;

  load(s0);
  store(&lds[0][0]);
  __syncthreads();

  for (int s = s0; s < s1; ++s) {
    const bool more = s + 1 < s1;
    if (more) load(s + 1);
    const int cur = ((s - s0) & 1) * kStage;
    if constexpr (TILE == 0) {
      f32x16 c;
#pragma unroll
      for (int e = 0; e < 16; ++e) c[e] = acc[e];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const bf16x8 af =
            __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(fa + cur + hh * 32));
        const bf16x8 bf =
            __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(fb + cur + hh * 32));
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, c, 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = c[e];
    } else {
      const bf16x8 af = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(fa + cur));
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16x8 bf = __builtin_bit_cast(
            bf16x8, *reinterpret_cast<const uint4*>(fb + cur + j * 16 * kRow));
        f32x4 c = {acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]};
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, c, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * j + e] = c[e];
      }
    }
    if (more) store(&lds[0][0] + (((s + 1 - s0) & 1) * kStage));
    __syncthreads();
  }

  // epilogue: for one e the lanes of a half (quarter) wave store consecutive columns
  float* const o = a.out + (a.partial ? (int64_t)sl * a.M * a.N : 0);
#pragma unroll
  for (int e = 0; e < NACC; ++e) {
    int m, n;
    if constexpr (TILE == 0) {
      m = m0 + wm * 32 + 4 * h + (e & 3) + 8 * (e >> 2);
      n = n0 + wn * 32 + lc;
    } else {
      m = m0 + 4 * h + (e & 3);
      n = n0 + wn * 32 + (e >> 2) * 16 + lc;
    }
    if (m < a.M && n < a.N) {
      float* const w = o + (int64_t)m * a.ldo + n;
      *w = (a.accumulate && !a.partial) ? *w + acc[e] : acc[e];
    }
  }
}

// C (+)= part[0] + part[1] + ... + part[S-1], in that order; C is not read
// without accumulate
__global__ void __launch_bounds__(kThreads)
gemm_bf16_sum_kernel(int64_t total, int N, int S, int accumulate, const float* __restrict__ part,
                     float* __restrict__ C, int64_t ldc) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  float t = part[i];
  for (int s = 1; s < S; ++s) t += part[s * total + i];
  float* const w = C + (i / N) * ldc + i % N;
  *w = accumulate ? *w + t : t;
}

// one thread per 16-byte piece of the packed matrix [N][Kp]
__global__ void __launch_bounds__(kThreads)
gemm_bf16_pack_kernel(int64_t pieces, int pieces_row, int K, const float* __restrict__ w,
                      int64_t ldw, uint4* __restrict__ packed) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= pieces) return;
  const int64_t row = q / pieces_row;
  const int k0 = (int)(q - row * pieces_row) * 8;
  unsigned v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = k0 + i < K ? bf16_rne(w[row * ldw + k0 + i]) : 0u;
  packed[q] = make_uint4(v[0] | v[1] << 16, v[2] | v[3] << 16, v[4] | v[5] << 16,
                         v[6] | v[7] << 16);
}

template <int FORM>
void launch_form(int tile, dim3 grid, const Bf16GemmArgs& a, hipStream_t s) {
  if (tile == 0)
    hipLaunchKernelGGL((gemm_bf16_kernel<FORM, 0>), grid, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((gemm_bf16_kernel<FORM, 1>), grid, dim3(kThreads), 0, s, a);
}

bool vec16(const float* p, int64_t ld) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0;
}

}  // namespace

int gemm_bf16_tile_count() { return 2; }

// The 16 x 128 tile where the 64-row one would be three quarters padding
int gemm_bf16_tile(int64_t M, int64_t forced) {
  if (forced >= 0) return (int)forced;
  return M <= 16 ? 1 : 0;
}

// The slices of the reduction (steps of 32): enough of them that the tiles x
// slices give each of the 256 CUs a block, none shorter than four steps, and
// the fp32 partials [S][M][N] within TNS_OPT_SCRATCH_CAP (cap > 0, in floats).
// forced >= 1 names the count; the result is clamped to the steps and
// normalised so that no slice is empty
int64_t gemm_bf16_split(int tile, int64_t M, int64_t N, int64_t K, int64_t forced, int64_t cap) {
  const int64_t bm = tile == 0 ? 64 : 16, bn = tile == 0 ? 64 : 128;
  const int64_t tiles = ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  const int64_t steps = std::max<int64_t>(1, (K + kStep - 1) / kStep);
  int64_t S = forced >= 1 ? forced : std::min((256 + tiles - 1) / tiles, steps / 4);
  if (cap > 0) S = std::min(S, cap / (M * N));
  S = std::max<int64_t>(1, std::min(S, steps));
  const int64_t per = (steps + S - 1) / S;
  return (steps + per - 1) / per;
}

int64_t gemm_bf16_packed_bytes(int64_t N, int64_t K) {
  return N * ((K + kStep - 1) / kStep * kStep) * 2;
}

hipError_t launch_gemm_bf16_pack(int64_t N, int64_t K, const float* W, int64_t ldw, void* packed,
                                 hipStream_t s) {
  const int64_t pieces = gemm_bf16_packed_bytes(N, K) / 16;
  const int64_t blocks = (pieces + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffLL || K > 0x7fffff00LL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gemm_bf16_pack_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, pieces,
                     (int)((K + kStep - 1) / kStep * 4), (int)K, W, ldw,
                     reinterpret_cast<uint4*>(packed));
  return hipGetLastError();
}

hipError_t launch_gemm_bf16(int tile, int split, const GemmBf16Args& g, hipStream_t s) {
  const int bm = tile == 0 ? 64 : 16, bn = tile == 0 ? 64 : 128;
  Bf16GemmArgs a{};
  a.A = g.A, a.B = static_cast<const float*>(g.B), a.lda = g.lda, a.ldb = g.ldb;
  a.M = (int)g.M, a.N = (int)g.N, a.K = (int)g.K;
  a.steps = (int)((g.K + kStep - 1) / kStep);
  // (the slices as the planner leaves them: none is empty)
  split = std::max(1, std::min(split, a.steps));
  a.per = (a.steps + split - 1) / split;
  split = (a.steps + a.per - 1) / a.per;
  a.mtiles = (int)((g.M + bm - 1) / bm);
  a.ntiles = (int)((g.N + bn - 1) / bn);
  a.partial = split > 1;
  a.accumulate = g.accumulate;
  a.out = a.partial ? g.part : g.C;
  a.ldo = a.partial ? g.N : g.ldc;
  a.va = vec16(g.A, g.lda), a.vb = vec16(a.B, g.ldb);
  const int64_t blocks = (int64_t)a.mtiles * a.ntiles * split;
  if (tile < 0 || tile >= gemm_bf16_tile_count() || blocks > 0x7fffffffLL ||
      (a.partial && !g.part))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks);
  switch (g.form) {
    case GEMM_BF16_NT: launch_form<FORM_NT>(tile, grid, a, s); break;
    case GEMM_BF16_TN: launch_form<FORM_TN>(tile, grid, a, s); break;
    case GEMM_BF16_NN: launch_form<FORM_NN>(tile, grid, a, s); break;
    case GEMM_BF16_NT_PACKED: launch_form<FORM_NTP>(tile, grid, a, s); break;
    default: return hipErrorInvalidValue;
  }
  if (hipError_t e = hipGetLastError(); e != hipSuccess || !a.partial) return e;
  const int64_t total = g.M * g.N;
  hipLaunchKernelGGL(gemm_bf16_sum_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, total, a.N, split, a.accumulate, g.part, g.C, g.ldc);
  return hipGetLastError();
}

}  // namespace tns

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
