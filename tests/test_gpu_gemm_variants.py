"""Every SGEMM kernel instantiation on the GPU, bit for bit against the oracle.

The cases are data (tests/_gemm_cases.py); tests/test_gemm_plan.py checks
without a GPU that between them they reach every leaf of the GEMM planner.

Every case
  * writes C inside a larger buffer: ldc = N + 3 unless the case needs
    another, the value -77.25 before C, after C, between the images and in
    every row's padding, all of it bit-identical after the call;
  * takes its inputs from uniform(-1, 1) of a generator seeded by the case id;
  * compares with np.array_equal (equal_nan where C0 holds a NaN);
  * must run where the support table (_gemm_cases.supported: the KIND column
    and the `applies` comments) says the variant takes the problem, and must
    raise TnsError and leave C untouched where it says it does not;
and each test asserts how many cases ran and how many were refused.

Reference.  NN and TN: the oracle's sgemm.  NT and TT through sgemm_kernel.hpp's
MFMA tile (a forced variant, TNS_OPT_NT_SDOT = 0, TNS_OPT_TT_EXACT = 0): the
oracle's sgemm with transB = false on a materialised contiguous B^T, i.e. the
ascending-k fmaf chain from beta*C with A pre-multiplied by alpha that
sgemm_kernel.hpp promises for every transpose (the oracle's own NT / TT orders
differ from it at these shapes: test_gemm_plan.py checks that on the CPU).
Every other path: the oracle's sgemm in the call's own transposes.
"""
from contextlib import contextmanager

import numpy as np
import pytest

from _gemm_cases import (NN_BIG, TILES, VARIANT_NAMES, SENT, batch_cases, leaf_cases,
                         matrix_cases, option_cases, supported, sweep_cases)

pytestmark = pytest.mark.gpu

SENT_BITS = int(np.float32(SENT).view(np.int32))


@contextmanager
def options(hiplib, c):
    """The case's process-wide options, the defaults again afterwards."""
    try:
        hiplib.tns_set_option(0, int(c.strict))
        hiplib.tns_set_option(3, c.nt_sdot)
        hiplib.tns_set_option(5, c.tt_exact)
        hiplib.tns_set_option(6, c.sdot_form)
        yield
    finally:
        hiplib.tns_set_option(0, 1)
        hiplib.tns_set_option(3, 1)
        hiplib.tns_set_option(5, 1)
        hiplib.tns_set_option(6, -1)


def operands(c):
    rng = np.random.default_rng(c.seed)
    nA = c.offA + (c.batch - 1) * c.SA + c.rowsA * c.LDA + 1
    nB = c.offB + (c.batch - 1) * c.SB + c.rowsB * c.LDB + 1
    A = rng.uniform(-1, 1, nA).astype(np.float32)
    B = rng.uniform(-1, 1, nB).astype(np.float32)
    C0 = rng.uniform(-1, 1, (c.batch, c.M, c.N)).astype(np.float32)
    if c.nan_c:
        C0[0, c.M // 2, c.N // 3] = np.nan
        C0[-1, c.M - 1, 0] = np.inf
    return A, B, C0


def reference(ora, c, A, B, C0):
    """C after the call, [batch][M][N] (only c.rows of each image where the
    case samples rows)."""
    ref = C0.copy()
    if c.beta == 0.0 and not c.strict:
        ref[:] = 0  # BLAS convention: C is not read
    asc = c.forced_mfma and c.tb and c.K > 0
    if c.batch > 1 and not asc and not c.rows:  # the oracle's own strided-batched loop
        ora.sgemm_batch_strided(bool(c.ta), bool(c.tb), c.M, c.N, c.K, c.alpha, A[c.offA:], c.LDA,
                                c.SA, B[c.offB:], c.LDB, c.SB, c.beta, ref, c.N, c.M * c.N,
                                c.batch)
        return ref
    for b in range(c.batch):
        a = A[c.offA + b * c.SA:]
        bm = B[c.offB + b * c.SB:]
        tb, ldb = bool(c.tb), c.LDB
        if asc:  # one ascending chain: NN / TN on B^T
            bm = np.ascontiguousarray(bm[:c.N * c.LDB].reshape(c.N, c.LDB)[:, :c.K].T)
            tb, ldb = False, c.N
        if c.rows:
            for r in c.rows:
                ora.sgemm_rows(bool(c.ta), tb, r, r + 1, c.M, c.N, c.K, c.alpha, a, c.LDA, bm, ldb,
                               c.beta, ref[b], c.N)
        else:
            ora.sgemm(bool(c.ta), tb, c.M, c.N, c.K, c.alpha, a, c.LDA, bm, ldb, c.beta, ref[b],
                      c.N)
    return ref


def run_case(hip, hiplib, T, ora, c):
    """Runs c; returns True if it ran, False if it was refused (both checked
    against the support table)."""
    from tensorium_amd._abi import TnsError
    A, B, C0 = operands(c)
    dA, dB = T.from_numpy(A).cuda(), T.from_numpy(B).cuda()
    nC = c.offC + (c.batch - 1) * c.SC + (c.M - 1) * c.LDC + c.N + 7
    dC = T.full((nC,), float(SENT), dtype=T.float32, device="cuda")
    view = T.as_strided(dC, (c.batch, c.M, c.N), (c.SC, c.LDC, 1), c.offC)
    view.copy_(T.from_numpy(C0).cuda())

    def call():
        pa, pb = (None, None) if c.null_ab else (dA, dB)
        if c.variant >= 0:
            hip.gemmVariant(c.variant, c.ta, c.tb, c.M, c.N, c.K, c.alpha, pa, c.offA, c.LDA, c.SA,
                            pb, c.offB, c.LDB, c.SB, c.beta, dC, c.offC, c.LDC, c.SC, c.batch)
        else:
            hip.gemmStridedBatched(c.ta, c.tb, c.M, c.N, c.K, c.alpha, pa, c.offA, c.LDA, c.SA, pb,
                                   c.offB, c.LDB, c.SB, c.beta, dC, c.offC, c.LDC, c.SC, c.batch)
        hip.finish()

    with options(hiplib, c):
        if supported(c):
            call()  # (a TnsError here fails the test: the table says supported)
            ran = True
        else:
            with pytest.raises(TnsError):
                call()
            hip.finish()
            ran = False
    got = view.cpu().numpy()
    view.fill_(float(SENT))
    assert not bool((dC.view(T.int32) != SENT_BITS).any()), (c.id, "a sentinel was overwritten")
    if not ran:
        assert np.array_equal(got.view(np.int32), C0.view(np.int32)), (c.id, "refused, C changed")
        return False
    ref = reference(ora, c, A, B, C0)
    nan = c.nan_c and c.strict
    if c.rows:
        rows = list(c.rows)
        assert np.array_equal(got[:, rows], ref[:, rows], equal_nan=nan), c.id
    else:
        bad = int((got.view(np.int32) != ref.view(np.int32)).sum()) if not nan else -1
        assert np.array_equal(got, ref, equal_nan=nan), (c.id, bad)
    if c.nan_c and not c.strict:
        assert np.isfinite(got).all(), (c.id, "the NaN of C0 must vanish")
    return True


def run_all(hip, hiplib, T, ora, cases):
    ran = sum(run_case(hip, hiplib, T, ora, c) for c in cases)
    return ran, len(cases) - ran


@pytest.mark.parametrize("v", range(len(TILES)), ids=[t[0] for t in TILES])
def test_instantiation_matrix(hip, hiplib, torch_cuda, ora, v):
    """Every instantiation of a table variant: launch_full's 4 transposes x 4
    stagings, launch_trans4's 4 transposes, launch_nn4's one and its refusals,
    each under the suite's (alpha, beta) pairs, a NaN and an Inf in C0 under
    strict beta = 0 and the same NaN with strict mode off."""
    from tensorium_amd._abi import gemm_plan
    cases = matrix_cases(v)
    for c in cases:  # the staging the case means is the one the library plans
        p = gemm_plan(**c.plan_args())
        assert (p["vec_a"], p["vec_b"]) == (4 if c.vecA() else 1, 4 if c.vecB() else 1), c.id
    counts = run_all(hip, hiplib, torch_cuda, ora, cases)
    assert counts == {"full": (80, 0), "trans4": (20, 1), "nn4": (5, 4)}[TILES[v][5]]


@pytest.mark.parametrize("v", range(len(TILES)), ids=[t[0] for t in TILES])
def test_k_and_edge_sweep(hip, hiplib, torch_cuda, ora, v):
    """K in {0, 1, BK - 1, BK, BK + 1} (K = 0 with null A and B: beta * C0) x
    (M, N) in {(1, 1), (BM, BN), (BM + 1, BN + 1), (MF - 1, MF + 1)}, every
    transpose the KIND has.  A float4-only variant takes the sizes that are
    multiples of 4 and refuses the others."""
    cases = sweep_cases(v)
    want = sum(supported(c) for c in cases)
    counts = run_all(hip, hiplib, torch_cuda, ora, cases)
    assert counts == (want, len(cases) - want)
    # what a float4-only variant takes: the contiguous extents must be
    # multiples of 4.  NN: K in {0, BK} at (BM, BN): 2.  NT (both extents are
    # K): K in {0, BK} at every (M, N): 8.  TN (extents M and N): (BM, BN) at
    # every K: 5.  TT (extents M and K): K in {0, BK} at (BM, BN): 2.
    assert counts == {"full": (80, 0), "trans4": (17, 63), "nn4": (2, 18)}[TILES[v][5]]


@pytest.mark.parametrize("v", range(len(VARIANT_NAMES)), ids=VARIANT_NAMES)
def test_batches(hip, hiplib, torch_cuda, ora, v):
    """batch = 3 with A shared (strideA = 0), padded strides for B and C and an
    element offset on every operand, against the oracle's strided-batched
    loop (the per-image sgemm of `reference`)."""
    cases = batch_cases(v)
    kind = TILES[v][5] if v < len(TILES) else "nn_big"
    assert run_all(hip, hiplib, torch_cuda, ora, cases) == \
        {"full": (4, 0), "trans4": (2, 0), "nn4": (1, 0), "nn_big": (1, 0)}[kind]


def test_mfma_transposes_through_options(hip, hiplib, torch_cuda, ora):
    """TNS_OPT_NT_SDOT = 0 and TNS_OPT_TT_EXACT = 0 at default dispatch, on
    every tile pick_tile_variant returns for a transposed B: bit-identical to
    the ascending chain."""
    from tensorium_amd._abi import gemm_plan
    cases = option_cases()
    for c, tile in cases:
        p = gemm_plan(**c.plan_args())
        assert (p["family"], p["name"]) == ("tile", tile), (c.id, p)
    assert {tile for _, tile in cases} == {"32x256x32_w1x4", "64x256x32_w1x4", "256x256x32_w2x4",
                                           "64x128x32_w2x2", "128x64x32_w2x2"}
    assert run_all(hip, hiplib, torch_cuda, ora, [c for c, _ in cases]) == (10, 0)


LEAF_CASES = leaf_cases()


@pytest.mark.parametrize("c,leaf", LEAF_CASES, ids=[c.id for c, _ in LEAF_CASES])
def test_remaining_leaves(hip, hiplib, torch_cuda, ora, c, leaf):
    """One case per plan leaf nothing above reaches: the large-NN cascade, every
    launch_sgemm_nt_sdot leaf, the tt kernel.  The shape was found by asking
    the planner; that it still gives the leaf is asserted first."""
    from tensorium_amd._abi import gemm_plan
    p = gemm_plan(**c.plan_args())
    assert (p["err"], p["leaf"]) == (0, leaf), p
    assert run_case(hip, hiplib, torch_cuda, ora, c)


def test_large_nn_forms_refuse_what_applies_excludes(hip, hiplib, torch_cuda, ora):
    """A large-NN form forced on a problem its `applies` rule excludes (a
    ragged M, a K that is no multiple of the k-tile, a transposed operand, a
    misaligned A) raises and leaves C untouched."""
    from _gemm_cases import Case
    nb, ran = len(TILES), 0
    cases = []
    for f, (name, bm, bn, bk, _) in enumerate(NN_BIG):
        ok = Case(f"refuse/{name}/ok", 0, 0, bm, bn, 2 * bk, variant=nb + f, alpha=0.5, beta=2.0)
        cases += [ok, Case(f"refuse/{name}/m", 0, 0, bm + 4, bn, 2 * bk, variant=nb + f),
                  Case(f"refuse/{name}/k", 0, 0, bm, bn, 2 * bk + 4, variant=nb + f),
                  Case(f"refuse/{name}/tn", 1, 0, bm, bn, 2 * bk, variant=nb + f),
                  Case(f"refuse/{name}/ptr", 0, 0, bm, bn, 2 * bk, variant=nb + f, offA=1)]
    assert run_all(hip, hiplib, torch_cuda, ora, cases) == (len(NN_BIG), 4 * len(NN_BIG))
