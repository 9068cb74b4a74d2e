// sgemm_nn_w4.hip — large aligned gemm(NoTrans, NoTrans), one wave per SIMD.
//
// The 256 x 256 x 32 block of sgemm_nn_big.hip / sgemm_nn_pp.hip with the
// same arithmetic (the reference's cblas_sgemm -> s_nn over saxpy_avx2,
// ntensors.pas:2061-2157, 2231-2286: every C element an ascending-k fma chain
// from beta*C, A_PART = ALPHA*A rounded once; v_mfma_f32_32x32x2_f32 step s
// consumes k = 2s + h, lane half h), so bit-identical to them; the block is
// laid out for one wave per SIMD instead of two:
//
//   * 4 waves (2 x 2), wave tile 128 x 128 = 4 x 4 accumulators of 32 x 32
//     (256 accumulator registers per lane: the wave has the SIMD's whole
//     register file to itself), so a step is 16 MFMAs = 1024 matrix-pipe
//     cycles fed by two ds_read2st64_b32 of A and one ds_read_b128 of B — no
//     partner wave's staging on the SIMD;
//   * BOTH operands stream global -> LDS by LDS-DMA (global_load_lds_dwordx4,
//     SGPR base + one per-lane VGPR offset for the whole launch): no staging
//     registers, no VALU transposes, no ds_write;
//   * A lands as row images [m][32 k] whose 16-byte k-chunks are XOR-swizzled
//     by row on the source side (chunk slot = chunk ^ ((m >> 1) & 7)), B as
//     [k][256 n] rows rotated by 32 floats on odd k: both fragment reads are
//     conflict-free or 2-way (A: lanes m and m + 16 share a bank);
//   * two LDS stages (2 x 64 KB); the barrier that publishes tile t+1 sits
//     before tile t's last step, whose 16 MFMAs each carry one of the 16 DMA
//     instructions of tile t+2 (into tile t's stage): the DMA goes out a whole
//     tile ahead of its use; fragments of step s+1 are read before step s's
//     MFMAs (scheduling fences);
//   * interleaved columns: accumulator tile j's column lc is block column
//     wn*128 + 4 lc + j (not 32 j + lc), so a lane's four B fragments of a
//     step are one ds_read_b128 and its four tiles' values of one row are 4
//     consecutive columns of C: beta loads and epilogue stores move 16 bytes
//     per lane.
//
// Measured at 4096^3 (scripts/nn_big_ab.py, profiles/r04_sgemm_w4_ab.json): 0.950 ms
// vs 0.983 for the ping-pong form on the same box, bit-identical.  (The
// forms with 32 j + lc columns and 4-byte B reads, with the DMA issued as one
// burst, measured 0.988-0.992 ms and did not reproduce the ping-pong bits at
// 4096^3; dropped.)
//
// alpha != 1 multiplies the A fragments after the read (one rounding, as the
// reference's A_PART = ALPHA*A[kk]).
//
// Two schedules of the same chains (template parameter ROWS):
//
//   * flat: every step runs all 16 accumulators.  The block loads its whole
//     256 KB of beta*C before its first MFMA and stores 256 KB after its last.
//   * rows (K >= 128): the first two and the last two k-tiles run one
//     accumulator row (4 of the 16 tiles: 32 rows of the wave tile) at a time,
//     a (row, tile) unit being 16 steps of one A read, the b128 B read and 4
//     MFMAs.  Front: the DMA of tile 0 and the C loads of row 0 go out first;
//     the MFMAs start when those have landed, rows 1-3 of C land under them
//     (two 64-register staging sets, counted vmcnt on the in-order counter
//     the C loads share with the DMA).  Unit order r0t0 r0t1 r1t0 r1t1 r2t0
//     r3t0 | r2t1 r3t1: tile 0's stage is free two units before the regular
//     loop, and takes tile 2's DMA under r2t1.  Back: r0 r1 of tile nt-2 (so
//     tile nt-1's DMA has two units to land), then each row's tile nt-1
//     followed by its 16 stores, issued one per step under the next unit's
//     MFMAs: only row 3's stores have nothing to hide under.  Between the
//     ends the flat loop runs unchanged.  Only the interleaving of
//     independent accumulators differs, so the bits are the flat schedule's.
//     With the accumulators starting from zero (BLAS beta = 0) the front is
//     the flat one.
//
// Rows against flat, same process and box, warm clock, interleaved rounds
// (scripts/nn_big_ab.py --variants 7,6; profiles/sgemm_w4_rows_ab.json), medians,
// bit-identical everywhere:
//   4096^3        strict beta = 0  0.9545 -> 0.9393 ms (0.984; flat spread 0.0006)
//                 beta = 1         0.9589 -> 0.9442      BLAS beta = 0  0.9458 -> 0.9320
//   1024 x 1024^3 strict beta = 0  16.37 -> 16.09 ms (0.983)   BLAS  15.81 -> 15.60
//   4096 x 4096 x K, strict: K = 128 0.0527 -> 0.0453 (0.858), 256 0.0817 ->
//                 0.0744, 512 0.1394 -> 0.1316; K = 128 BLAS 0.0430 -> 0.0385
// so rows is what launch_sgemm_nn_w4 runs wherever K >= 128.  Per-wave s_memtime
// stamps (-DTNS_W4_STAMPS, scripts/w4_stamps.py, profiles/sgemm_w4_rows_stamps.json),
// medians at 4096^3: entry -> first MFMA 28.5 k cycles flat (12 us: the whole
// 384 KB prologue of a block) -> 17.4 k rows (tile 0 + C row 0: 128 KB); last
// MFMA -> last store done 12.0 k flat (5.1 us: the exposed store) -> 1.5 k; at
// 1024 x 1024^3 29.9 k -> 23.4 k and 6.3 k -> 1.3 k.  The estimate was up to 17
// us a tile; found: 15 us a launch at 4096^3 (the stamps put 4.7 us of it
// before the first MFMA and 4.5 us after the last; the rest lies inside the
// MFMA span, which the stamps do not split), 4.5 us a tile at config 4, whose
// blocks are not in step, so part of their C traffic already ran beside
// other CUs' loops.
//
// Fragment addresses (template parameter PRE).  With one wave per SIMD every
// instruction between two MFMAs is paid for in issue time (scripts/w4_probe.hip,
// profiles/sgemm_w4_afrag_probe.json: eight v_nop in front of a step cost what
// eight v_mul_f32 do, 0.07 of the 0.09 ms between operands in registers and
// the LDS reads; the same reads with no address arithmetic run within 0.01 ms
// of the registers; 8-byte A reads with v_permlane32_swap, and the reads
// spread over the MFMA gaps, measured slower and were not kept).  The XOR
// swizzle and the run-time stage kept the A address out of the instruction
// offset: 1.5 VALU a step and SALU beside them.  PRE computes the lane's 16 A
// addresses (8 chunks x 2 k-pairs) of each stage and its B base once in front
// of the regular loop and runs two tiles an iteration, one per stage, and an
// odd last one: a step is its three LDS reads and one wait.  The rows
// schedule's ends keep the per-step arithmetic.  Same values, same chains.
// A/B against the per-step arithmetic (scripts/nn_big_ab.py --variants 8,6;
// profiles/sgemm_w4_afrag_ab.json), medians, bit-identical everywhere:
//   4096^3        strict beta = 0  0.9364 -> 0.9167 ms (0.979; 12.5 x the 0.0016 spread)
//                 beta = 1         0.9337 -> 0.9167      BLAS beta = 0  0.9269 -> 0.9099
//   1024 x 1024^3 strict beta = 0  16.06 -> 15.86 ms (0.988)
//   4096 x 4096 x K, strict: K = 512 0.1317 -> 0.1308; 160 .. 384 level; K = 128
//                 (no regular tile) 0.0451 -> 0.0456, slower: see PRE_MIN_TILES
// 444 VGPRs with the 256 accumulators, no spill, code 40.5 -> 49.4 KB.
#include <type_traits>

#include "tns_internal.hpp"

namespace tns {
namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef int int4v __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(3))) float* lds_cptr;
typedef const __attribute__((address_space(3))) floatx4* lds_cptr4;

constexpr int BM = 256, BN = 256, BK = 32, NT = 256;
constexpr int A_TILE = BM * BK, B_TILE = BK * BN, STAGE = A_TILE + B_TILE;  // floats
constexpr int ROWS_MIN_TILES = kW4RowsMinTiles;  // the rows schedule's two ends are two k-tiles each
// the picked (rows) form holds its loop's fragment addresses in registers from
// this many k-tiles on: measured slower below (K = 128, no regular tile, by
// 0.5 us), level from 160 to 384, faster from 512
constexpr int PRE_MIN_TILES = kW4PreMinTiles;

__device__ __forceinline__ void dma16(const float* sbase, unsigned voff, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds)
      : "memory");
}

#ifdef TNS_W4_STAMPS
// diagnostic build only: s_memtime of every wave at entry, first MFMA, last
// MFMA and after its last store has completed (4 x 64 bits per wave)
#define TNS_W4_STAMP(i) stamp[i] = __builtin_amdgcn_s_memtime()
#else
#define TNS_W4_STAMP(i) \
  do {                  \
  } while (0)
#endif

template <bool ALPHA1, bool ROWS, bool PRE>
__global__ __launch_bounds__(NT, 1) void sgemm_nn_w4_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
#ifdef TNS_W4_STAMPS
  unsigned long long stamp[4];
  TNS_W4_STAMP(0);
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lc = lane & 31, h = lane >> 5;
  const int wm = wid >> 1, wn = wid & 1;

  // XCD-contiguous grouped raster (as sgemm_nn_big.hip)
  const int tiles_m = (int)(p.M / BM), tiles_n = (int)(p.N / BN);
  int tm, tn;
  const int64_t bz = blockIdx.y;
  {
    const int nb = tiles_m * tiles_n, bid = blockIdx.x;
    const int xcd = bid & 7, q = nb >> 3, r = nb & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    constexpr int GROUP_M = 8;
    const int per_group = GROUP_M * tiles_n;
    const int group = wg / per_group, first_m = group * GROUP_M;
    const int gsize = min(tiles_m - first_m, GROUP_M);
    const int in_group = wg - group * per_group;
    tm = first_m + in_group % gsize;
    tn = in_group / gsize;
  }
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const float* __restrict__ A = p.A + bz * p.strideA;
  const float* __restrict__ B = p.B + bz * p.strideB;
  float* __restrict__ C = p.C + bz * p.strideC;
  const int64_t lda = p.lda, ldb = p.ldb, ldc = p.ldc;

  // ---- LDS-DMA staging: wave w moves A row groups 8q..8q+7 (q = 8w + u,
  // u < 8: 1 KB each) and B k-rows r = 8w + u of a tile ----------------------
  // A: lane i -> row 8q + (i >> 3), LDS chunk slot i & 7 <- k-chunk
  //    (i & 7) ^ ((row >> 1) & 7)
  // B: lane i -> LDS chunk i of row r <- n-chunk (i + 8 (r & 1)) & 63
  const int arow = lane >> 3;  // row within the group (group rows are 8-aligned)
  const unsigned a_voff = (unsigned)(arow * lda * 4) + 16u * (unsigned)((lane & 7) ^ ((arow >> 1) & 7));
  // ((8q + arow) >> 1) & 7 = (4q + (arow >> 1)) & 7: q even -> (arow >> 1),
  // q odd -> (arow >> 1) ^ 4; odd groups use the second offset
  const unsigned a_voff1 = (unsigned)(arow * lda * 4) +
                           16u * (unsigned)((lane & 7) ^ (((arow >> 1) & 7) ^ 4));
  const unsigned b_voff0 = 16u * (unsigned)lane;
  const unsigned b_voff1 = 16u * (unsigned)((lane + 8) & 63);
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)smem;
  const float* a_row0 = A + m0 * lda;  // + (8q) * lda + k0
  const float* b_row0 = B + n0;        // + (k0 + r) * ldb
  // DMA instruction u (0..15) of this wave for tile k0 into stage st
  auto issue1 = [&](int u, int64_t k0, int st) {
    const unsigned sb = lds0 + (unsigned)(st * STAGE * 4);
    if (u < 8) {
      const int q = 8 * wid + u;
      dma16(a_row0 + (int64_t)(8 * q) * lda + k0, (u & 1) ? a_voff1 : a_voff,
            sb + (unsigned)(q * 1024));
    } else {
      const int r = 8 * wid + (u - 8);
      dma16(b_row0 + (k0 + r) * ldb, (u & 1) ? b_voff1 : b_voff0,
            sb + (unsigned)(A_TILE * 4 + r * 1024));
    }
  };
  auto issue = [&](int64_t k0, int st) {
    const unsigned sb = lds0 + (unsigned)(st * STAGE * 4);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int q = 8 * wid + u;
      dma16(a_row0 + (int64_t)(8 * q) * lda + k0, (u & 1) ? a_voff1 : a_voff,
            sb + (unsigned)(q * 1024));
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = 8 * wid + u;
      dma16(b_row0 + (k0 + r) * ldb, (u & 1) ? b_voff1 : b_voff0,
            sb + (unsigned)(A_TILE * 4 + r * 1024));
    }
  };

  const int nt = (int)(p.K / BK);

  // ---- accumulators and C addressing ----------------------------------------
  // C through a buffer resource over this block's rows: the lane's column in
  // a 32-bit VGPR offset, the row (wave-uniform: i, e) in the SGPR offset,
  // the column tile j in the instruction offset — no 64-bit row addresses
  // held across the loop
  floatx16 acc[4][4];
  const int64_t row_base = m0 + wm * 128;
  const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc(
      C + row_base * ldc, 0, 0x7fffffff, 0x00020000);
  const unsigned c_voff = 4u * (unsigned)(4 * h * ldc + n0 + wn * 128 + 4 * lc);
  auto c_soff = [&](int i, int e) {
    return (unsigned)(4 * (32 * i + (e & 3) + 8 * (e >> 2)) * ldc);
  };

  // ---- fragments: step s (k = 2s + h) --------------------------------------
  // A tile i: row wm*128 + 32 i + lc, chunk (k >> 2) ^ swz, swz = (lc >> 1) & 7
  // B tile j: n = wn*128 + 32 j + lc at LDS column (n - 32 h) & 255 of row k
  const int swz = (lc >> 1) & 7;
  int b_col[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    b_col[j] = A_TILE + h * BN + ((wn * 128 + 4 * lc + j - 32 * h) & 255);
  const float alpha = p.alpha;
  auto mma = [&](const float (&a)[4], const float (&b)[4]) {
    float aa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) aa[i] = ALPHA1 ? a[i] : alpha * a[i];  // A_PART = ALPHA*A
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[i], b[j], acc[i][j], 0, 0, 0);
  };
  // a step's 16 MFMAs with the 16 DMA instructions of tile k0 issued
  // one after each: the DMA issue (SALU + VMEM) fills the 64-cycle gaps the
  // matrix pipe leaves between this wave's MFMAs instead of delaying them
  auto mma_dma = [&](const float (&a)[4], const float (&b)[4], int64_t k0, int st, bool dma) {
    float aa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) aa[i] = ALPHA1 ? a[i] : alpha * a[i];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = u >> 2, j = u & 3;
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[i], b[j], acc[i][j], 0, 0, 0);
      if (dma) issue1(u, k0, st);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  const int a_lane = (wm * 128 + lc) * BK + h;
  auto frag = [&](const float* st, int s, float (&a)[4], float (&b)[4]) {
    const int ka = 4 * ((s >> 1) ^ swz) + 2 * (s & 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = st[a_lane + 32 * BK * i + ka];
    const floatx4 v = *reinterpret_cast<const floatx4*>(st + b_col[0] + 2 * s * BN);
    b[0] = v[0]; b[1] = v[1]; b[2] = v[2]; b[3] = v[3];
  };
  // PRE: the flat loop's fragment addresses held in registers, so that a step
  // issues its three LDS reads (two ds_read2st64_b32 of A, the b128 of B) and
  // no address arithmetic: per stage P the lane's A address of every k-chunk
  // j and k-pair o (the XOR swizzle and the + 2 floats are no instruction
  // offsets) and its B base.  Set up by pre_init() in front of the loop, whose
  // tiles then name their stage at compile time.
  lds_cptr ap[2][16], bp[2];
  auto pre_init = [&]() {
    // (computed from values made opaque here, so that none of the 34 is
    // hoisted above the front, where the C staging sets are live)
    int al = a_lane, sw = swz, bc = b_col[0];
    asm volatile("" : "+v"(al), "+v"(sw), "+v"(bc));
#pragma unroll
    for (int P = 0; P < 2; ++P) {
      const lds_cptr st = (lds_cptr)smem + P * STAGE;
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        ap[P][c] = st + al + 4 * ((c >> 1) ^ sw) + 2 * (c & 1);
        asm volatile("" : "+v"(ap[P][c]));
      }
      bp[P] = st + bc;
      asm volatile("" : "+v"(bp[P]));
    }
  };
  auto pfrag = [&](int P, int s, float (&a)[4], float (&b)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = ap[P][s][32 * BK * i];
    const floatx4 v = *reinterpret_cast<lds_cptr4>(bp[P] + 2 * s * BN);
    b[0] = v[0]; b[1] = v[1]; b[2] = v[2]; b[3] = v[3];
  };
  float a0[4], b0[4], a1[4], b1[4];
  // tile t on all 16 accumulators; a0/b0 hold its step 0 on entry.  The
  // barrier that publishes tile t+1 (pub) sits before step 15 of tile t, so
  // tile t+1's first fragments are read under step 15's MFMAs and the DMA of
  // tile t+2 (dma: into tile t's stage, whose reads all completed before the
  // barrier) goes out a whole tile ahead of its use
  // (P_: the tile's stage t & 1 as a constant; used by the PRE reads only)
  // (always_inline: called three times, it is otherwise left a function, the
  // accumulators passed through memory)
  auto flat_tile_p = [&](auto P_, int t, bool pub, bool dma) __attribute__((always_inline)) {
    constexpr int P = decltype(P_)::value;
    const float* cur = smem + (t & 1) * STAGE;
    const float* nxt = smem + ((t + 1) & 1) * STAGE;
    auto rd = [&](bool next, int s, float (&a)[4], float (&b)[4]) {
      if constexpr (PRE)
        pfrag(next ? 1 - P : P, s, a, b);
      else
        frag(next ? nxt : cur, s, a, b);
    };
#pragma unroll
    for (int s = 0; s < BK / 2 - 2; s += 2) {  // steps 0 .. 13
      rd(false, s + 1, a1, b1);
      __builtin_amdgcn_sched_barrier(0);
      mma(a0, b0);
      rd(false, s + 2, a0, b0);
      __builtin_amdgcn_sched_barrier(0);
      mma(a1, b1);
    }
    rd(false, BK / 2 - 1, a1, b1);  // step 15's fragments
    __builtin_amdgcn_sched_barrier(0);
    mma(a0, b0);                     // step 14
    __builtin_amdgcn_sched_barrier(0);
    if (pub) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of tile t+1
      __syncthreads();  // every wave's; every read of tile t complete
      rd(true, 0, a0, b0);
      __builtin_amdgcn_sched_barrier(0);
    }
    mma_dma(a1, b1, (int64_t)(t + 2) * BK, t & 1, dma);  // step 15 + tile t+2's DMA
  };
  // tiles t0 (even) .. t1-1; ALL: every tile publishes its successor and
  // issues the DMA of the one after (the rows schedule's loop), otherwise
  // where the product has them.  PRE runs two tiles an iteration, one per
  // stage, in straight line (two bodies behind a branch on t & 1 end in
  // accumulator spills), and an odd last one
  auto flat_loop = [&](auto ALL_, int t0, int t1) {
    constexpr bool ALL = decltype(ALL_)::value;
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    if constexpr (PRE) {
      int t = t0;
      for (; t + 1 < t1; t += 2) {
        flat_tile_p(P0{}, t, true, ALL || t + 2 < nt);
        flat_tile_p(P1{}, t + 1, ALL || t + 2 < nt, ALL || t + 3 < nt);
      }
      if (t < t1) flat_tile_p(P0{}, t, ALL || t + 1 < nt, ALL || t + 2 < nt);
    } else {
      for (int t = t0; t < t1; ++t) flat_tile_p(P0{}, t, ALL || t + 1 < nt, ALL || t + 2 < nt);
    }
  };

  if constexpr (!ROWS) {
    // the first two tiles' DMA goes out before the beta*C loads, so the two
    // latencies overlap (the C loads are younger: waiting for them waits for
    // the DMA too)
#ifdef TNS_W4_DMA_LATE  // (A/B side builds: round 4's order, DMA after the C loads)
    constexpr bool kDmaFirst = false;
#else
    constexpr bool kDmaFirst = true;
#endif
    if (kDmaFirst && nt > 0) issue(0, 0);
    if (kDmaFirst && nt > 1) issue(BK, 1);

    // ---- accumulators: 0, C or beta*C -------------------------------------
    if (p.beta_mode == BETA_ZERO) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    } else {
      // tile (i, j) = g: its 16 loads in flight while tile g-1 is moved into
      // its accumulator registers
      const bool scale = p.beta_mode == BETA_SCALE;
      const float beta = p.beta;
      {
        // row group g = (i, e-block of 4): 4 float4 loads = tiles 0..3 of 4 rows
        floatx4 v[2][4];
        auto ldv = [&](int g, floatx4 (&t)[4]) {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            t[u] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(
                                                   crs, c_voff, c_soff(g >> 2, 4 * (g & 3) + u), 0));
        };
        ldv(0, v[0]);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          if (g + 1 < 16) ldv(g + 1, v[(g + 1) & 1]);
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float c = v[g & 1][u][j];
              acc[g >> 2][j][4 * (g & 3) + u] = scale ? beta * c : c;
            }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(acc[i][j]));
    if (!kDmaFirst && nt > 0) issue(0, 0);
    if (!kDmaFirst && nt > 1) issue(BK, 1);

    if (nt > 0) {
      if (nt > 1) {
        // tile 0's 16 DMAs of this wave (with beta*C loaded: all of them)
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __syncthreads();
      if constexpr (PRE) {
        pre_init();
        pfrag(0, 0, a0, b0);
      } else {
        frag(smem, 0, a0, b0);
      }
    }
    TNS_W4_STAMP(1);
    flat_loop(std::false_type{}, 0, nt);
    TNS_W4_STAMP(2);

    // ---- epilogue --------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const floatx4 v = {acc[i][0][e], acc[i][1][e], acc[i][2][e], acc[i][3][e]};
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(int4v, v), crs, c_voff,
                                               c_soff(i, e), 0);
      }
  } else {
    // ---- rows schedule (nt >= ROWS_MIN_TILES) ---------------------------------
    // one accumulator row's fragments of step s: the A value of row i and the
    // b128 of B
    float fa0, fa1, fb0[4], fb1[4];
    auto rfrag = [&](const float* st, int s, int i, float& a, float (&b)[4]) {
      const int ka = 4 * ((s >> 1) ^ swz) + 2 * (s & 1);
      a = st[a_lane + 32 * BK * i + ka];
      const floatx4 v = *reinterpret_cast<const floatx4*>(st + b_col[0] + 2 * s * BN);
      b[0] = v[0]; b[1] = v[1]; b[2] = v[2]; b[3] = v[3];
    };
    auto rmma = [&](auto I_, float a, const float (&b)[4]) {
      constexpr int I = decltype(I_)::value;
      const float aa = ALPHA1 ? a : alpha * a;  // A_PART = ALPHA*A
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[I][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa, b[j], acc[I][j], 0, 0, 0);
    };
    // workgroup barrier that leaves VMEM (DMA, C loads, stores) in flight
    auto bar = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    auto none = [] {};
    auto none1 = [](int) {};
    using R0 = std::integral_constant<int, 0>;
    using R1 = std::integral_constant<int, 1>;
    using R2 = std::integral_constant<int, 2>;
    using R3 = std::integral_constant<int, 3>;
    using RN = std::integral_constant<int, -1>;
    // one (row, tile) unit: the 16 steps of the tile in stage st on accumulator
    // row I; fa0/fb0 hold its step 0 on entry.  after(s) follows step s's
    // MFMAs; mid() runs before step 15's (waits, barrier, C moves), then step 0
    // of the next unit (row NI of stage nst; RN: none) is read under them
    auto unit = [&](auto I_, const float* st, auto NI_, const float* nst, auto&& mid,
                    auto&& after) {
      constexpr int I = decltype(I_)::value, NI = decltype(NI_)::value;
#pragma unroll
      for (int s = 0; s < BK / 2 - 2; s += 2) {  // steps 0 .. 13
        rfrag(st, s + 1, I, fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        rmma(I_, fa0, fb0);
        after(s);
        rfrag(st, s + 2, I, fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);
        rmma(I_, fa1, fb1);
        after(s + 1);
      }
      rfrag(st, BK / 2 - 1, I, fa1, fb1);
      __builtin_amdgcn_sched_barrier(0);
      rmma(I_, fa0, fb0);  // step 14
      after(BK / 2 - 2);
      __builtin_amdgcn_sched_barrier(0);
      mid();
      if constexpr (NI >= 0) {
        rfrag(nst, 0, NI, fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);
      }
      rmma(I_, fa1, fb1);  // step 15
      after(BK / 2 - 1);
      __builtin_amdgcn_sched_barrier(0);
    };
    const float* const S0 = smem;
    const float* const S1 = smem + STAGE;

    int tb;  // first tile of the flat loop
    if (p.beta_mode == BETA_ZERO) {
      issue(0, 0);
      issue(BK, 1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
          asm volatile("" : "+a"(acc[i][j]));
        }
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");  // tile 0's DMA of this wave
      bar();
      TNS_W4_STAMP(1);
      tb = 0;
    } else {
      // ---- front: k-tiles 0 and 1 row by row under the beta*C loads ------------
      // The C loads are asm so that neither they nor the DMA are drained by a
      // compiler wait: the in-order VM counter holds, oldest first,
      //   T0 R0 T1 R1            (16 each: DMA of tile t, C of row i), then
      //   T1 R1 R2 -> R2 R3 -> R3 as rows are consumed and their staging set
      //   is loaded again.
      // Every wait names the registers it makes valid ("+v"), so no consumer
      // is scheduled above it.
      const bool scale = p.beta_mode == BETA_SCALE;
      const float beta = p.beta;
      const uint64_t cb = (uint64_t)(uintptr_t)(C + row_base * ldc);
      const int4v crs_raw = {(int)(uint32_t)cb, (int)((uint32_t)(cb >> 32) & 0xffffu), 0x7fffffff,
                             0x00020000};
      floatx4 va[16], vb[16];
      auto ldrow = [&](int i, floatx4 (&v)[16]) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const unsigned so = c_soff(i, e);
          if (e == 0)  // (s_nop: descriptor / offset SGPRs written just before)
            asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, %3 offen"
                         : "=&v"(v[e])
                         : "v"(c_voff), "s"(crs_raw), "s"(so)
                         : "memory");
          else
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen"
                         : "=&v"(v[e])
                         : "v"(c_voff), "s"(crs_raw), "s"(so)
                         : "memory");
        }
      };
      // wait until at most N younger VM operations are outstanding: v has landed
      auto waitrow = [&](auto N_, floatx4 (&v)[16]) {
        asm volatile("s_waitcnt vmcnt(%[n])"
                     : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]),
                       "+v"(v[6]), "+v"(v[7])
                     : [n] "n"(decltype(N_)::value)
                     : "memory");
        asm volatile(""
                     : "+v"(v[8]), "+v"(v[9]), "+v"(v[10]), "+v"(v[11]), "+v"(v[12]), "+v"(v[13]),
                       "+v"(v[14]), "+v"(v[15])
                     :
                     : "memory");
      };
      auto mvrow = [&](auto I_, const floatx4 (&v)[16]) {
        constexpr int I = decltype(I_)::value;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float c = v[e][j];
            acc[I][j][e] = scale ? beta * c : c;
          }
          asm volatile("" : "+a"(acc[I][j]));
        }
      };
      using N0 = std::integral_constant<int, 0>;
      using N16 = std::integral_constant<int, 16>;
      using N32 = std::integral_constant<int, 32>;

      issue(0, 0);
      ldrow(0, va);
      issue(BK, 1);
      ldrow(1, vb);
      waitrow(N32{}, va);  // T0 R0 landed
      bar();               // tile 0 published
      mvrow(R0{}, va);
      ldrow(2, va);
      rfrag(S0, 0, 0, fa0, fb0);
      __builtin_amdgcn_sched_barrier(0);
      TNS_W4_STAMP(1);
      unit(R0{}, S0, R0{}, S1, [&] {
        asm volatile("s_waitcnt vmcnt(32)" ::: "memory");  // T1 landed (R1 R2 may fly)
        bar();                                             // tile 1 published
      }, none1);
      unit(R0{}, S1, R1{}, S0, [&] {
        waitrow(N16{}, vb);  // R1 landed (R2 may fly)
        mvrow(R1{}, vb);
        ldrow(3, vb);
      }, none1);
      unit(R1{}, S0, R1{}, S1, none, none1);
      unit(R1{}, S1, R2{}, S0, [&] {
        waitrow(N16{}, va);  // R2 landed (R3 may fly)
        mvrow(R2{}, va);
      }, none1);
      unit(R2{}, S0, R3{}, S0, [&] {
        waitrow(N0{}, vb);  // R3 landed
        mvrow(R3{}, vb);
      }, none1);
      unit(R3{}, S0, R2{}, S1, none, none1);
      bar();  // every wave's reads of tile 0 complete: stage 0 takes tile 2,
              // two DMA instructions after each of r2t1's first 8 steps
      unit(R2{}, S1, R3{}, S1, none, [&](int s) {
        if (s < 8) {
          issue1(2 * s, 2 * BK, 0);
          issue1(2 * s + 1, 2 * BK, 0);
        }
      });
      unit(R3{}, S1, RN{}, S1, none, none1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of tile 2
      bar();  // tile 2 published; every wave's reads of tile 1 complete
      issue(3 * BK, 1);
      tb = 2;
    }

    // ---- tiles tb .. nt-3 on the flat schedule ------------------------------------
    const float* const sA = smem + (nt & 1) * STAGE;        // tile nt-2
    const float* const sB = smem + ((nt + 1) & 1) * STAGE;  // tile nt-1
    if (tb < nt - 2) {
      if constexpr (PRE) {  // (tb is even: stage 0)
        pre_init();
        pfrag(0, 0, a0, b0);
      } else {
        frag(S0, 0, a0, b0);
      }
      flat_loop(std::true_type{}, tb, nt - 2);
      fa0 = a0[0];  // row 0's step 0 of tile nt-2, read under the loop's last step
#pragma unroll
      for (int j = 0; j < 4; ++j) fb0[j] = b0[j];
    } else {
      rfrag(sA, 0, 0, fa0, fb0);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- back: tiles nt-2 and nt-1 row by row, each finished row's 16 stores
    // issued one per step under the next unit's MFMAs ------------------------------
    // (tile nt-2 is published and tile nt-1's DMA in flight here)
    auto store1 = [&](auto I_, int e) {
      constexpr int I = decltype(I_)::value;
      const floatx4 v = {acc[I][0][e], acc[I][1][e], acc[I][2][e], acc[I][3][e]};
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(int4v, v), crs, c_voff,
                                             c_soff(I, e), 0);
    };
    unit(R0{}, sA, R1{}, sA, none, none1);
    unit(R1{}, sA, R0{}, sB, [&] {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of tile nt-1
      bar();                                            // tile nt-1 published
    }, none1);
    unit(R0{}, sB, R1{}, sB, none, none1);
    unit(R1{}, sB, R2{}, sA, none, [&](int s) { store1(R0{}, s); });
    unit(R2{}, sA, R2{}, sB, none, [&](int s) { store1(R1{}, s); });
    unit(R2{}, sB, R3{}, sA, none, none1);
    unit(R3{}, sA, R3{}, sB, none, [&](int s) { store1(R2{}, s); });
    unit(R3{}, sB, RN{}, sB, none, none1);
    TNS_W4_STAMP(2);
#pragma unroll
    for (int e = 0; e < 16; ++e) store1(R3{}, e);
  }
#ifdef TNS_W4_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores done
  TNS_W4_STAMP(3);
  const unsigned blk = blockIdx.y * gridDim.x + blockIdx.x;
  if (lane == 0 && p.stamps != nullptr && blk < (1u << 16)) {
    unsigned long long* d = reinterpret_cast<unsigned long long*>(p.stamps) + (4 * blk + wid) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = stamp[i];
  }
#endif
}

#ifdef TNS_W4_STAMPS
unsigned* g_w4_stamps = nullptr;
#endif

}  // namespace

static_assert(BM == kNnBigGeo[6].bm && BN == kNnBigGeo[6].bn && BK == kNnBigGeo[6].bk &&
              kNnBigGeo[6].off32, "forms 6..8 of kNnBigGeo are this tile");

// the plan (plan_gemm_variant, gemm_plan.cpp) says the form applies and gives
// the kernel's template arguments:
// rows: the row-ordered schedule of the first and last two k-tiles where K
// has them (K >= 128), the flat schedule below that
// pre: the flat loop reads its fragments from addresses held in registers
// (the kernel's PRE; with rows only where K >= 256, see PRE_MIN_TILES); false
// keeps the per-step address arithmetic, for A/B
hipError_t launch_sgemm_nn_w4(const GemmPlan& p, const GemmArgs& a, hipStream_t s) {
  if (p.err || p.family != GEMM_NN_BIG || p.form < 6) return hipErrorInvalidValue;
  const bool rows = p.rows, pre = p.pre, alpha1 = p.alpha1;
  const int64_t tiles = (a.M / BM) * (a.N / BN);
  for (int64_t b0 = 0; b0 < a.batch; b0 += 65535) {
    GemmArgs sub = a;
    const int64_t nb = a.batch - b0 < 65535 ? a.batch - b0 : 65535;
    sub.A = a.A + b0 * a.strideA;
    sub.B = a.B + b0 * a.strideB;
    sub.C = a.C + b0 * a.strideC;
    sub.batch = nb;
#ifdef TNS_W4_STAMPS
    sub.stamps = g_w4_stamps;
#endif
    const dim3 grid((unsigned)tiles, (unsigned)nb);
    auto go = [&](auto R_, auto P_) {
      constexpr bool R = decltype(R_)::value, P = decltype(P_)::value;
      if (alpha1)
        hipLaunchKernelGGL((sgemm_nn_w4_kernel<true, R, P>), grid, dim3(NT), 0, s, sub);
      else
        hipLaunchKernelGGL((sgemm_nn_w4_kernel<false, R, P>), grid, dim3(NT), 0, s, sub);
    };
    if (rows && pre)
      go(std::true_type{}, std::true_type{});
    else if (rows)
      go(std::true_type{}, std::false_type{});
    else if (pre)
      go(std::false_type{}, std::true_type{});
    else
      go(std::false_type{}, std::false_type{});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

#ifdef TNS_W4_STAMPS
// diagnostic build only (not in include/tns.h): every wave's four stamps into
// dev_buf (4 x 64 bits per wave, 4 waves per block, the first 65536 blocks),
// or nothing when NULL
extern "C" int tns_debug_w4_stamps(unsigned* dev_buf) {
  g_w4_stamps = dev_buf;
  return 0;
}
#endif

}  // namespace tns
