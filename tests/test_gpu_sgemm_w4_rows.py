"""The one-wave-per-SIMD large-NN SGEMM (sgemm_nn_w4.hip) on its two schedules,
forced through gemmVariant: the row-ordered one (first and last two k-tiles one
accumulator row at a time, C loads and stores under the MFMAs; flat below
K = 128) and the flat one.  Both run the reference's ascending-k fma chain
from beta*C per element, so every case is compared with the oracle bit for
bit: NaNs in the same places, and the same uint32 words wherever the
reference is finite (the sign of zero counts).

Shapes are the smallest at which the schedule can go wrong: one block and two,
K = 32 .. 192 = 1 .. 6 k-tiles (flat fallback below 4; front and back adjacent
at 4; one and two regular tiles between them at 5 and 6).
"""
import numpy as np
import pytest

from tensorium_amd._abi import TNS_OPT_STRICT_BETA0

pytestmark = pytest.mark.gpu

ROWS = "256x256x32_w2x2_dma_nn_big"
FLAT = "256x256x32_w2x2_dma_flat_nn_big"
KS = [32, 64, 96, 128, 160, 192]
MODES = [(1.0, 0.0), (1.0, 1.0), (0.5, 2.0), (-1.5, 0.25)]


def forms(hip):
    names = hip.gemmVariants()
    return [names.index(ROWS), names.index(FLAT)]


def assert_bits(got, ref, what):
    assert np.array_equal(got, ref, equal_nan=True), what
    fin = np.isfinite(ref)
    assert np.array_equal(got.view(np.uint32)[fin], ref.view(np.uint32)[fin]), what


def run_form(hip, torch, v, A, B, C0, alpha, beta):
    M, N = C0.shape
    K = A.shape[1]
    dA, dB, dC = (torch.from_numpy(x).cuda() for x in (A, B, C0.copy()))
    hip.gemmVariant(v, False, False, M, N, K, alpha, dA, 0, K, 0, dB, 0, N, 0, beta, dC, 0, N, 0, 1)
    hip.finish()
    return dC.cpu().numpy()


def reference(ora, A, B, C0, alpha, beta):
    M, N = C0.shape
    K = A.shape[1]
    C = C0.copy()
    ora.sgemm(False, False, M, N, K, alpha, A, K, B, N, beta, C, N)
    return C


def operands(seed, M, N, K):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    B = rng.uniform(-1, 1, (K, N)).astype(np.float32)
    C0 = rng.uniform(-1, 1, (M, N)).astype(np.float32)
    return A, B, C0


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,N", [(256, 256), (512, 256)])
def test_k_sweep_every_beta_mode(hip, torch_cuda, ora, M, N, K):
    """nt = 1 .. 6 k-tiles under strict beta = 0, beta = 1, two scaled modes
    with alpha != 1, and the BLAS beta = 0 convention (C not read: the NaNs
    left in it must not reach the result)."""
    A, B, C0 = operands(1000 * M + K, M, N, K)
    for alpha, beta in MODES:
        ref = reference(ora, A, B, C0, alpha, beta)
        for v in forms(hip):
            assert_bits(run_form(hip, torch_cuda, v, A, B, C0, alpha, beta), ref,
                        (v, M, N, K, alpha, beta))
    ref = reference(ora, A, B, np.zeros_like(C0), 1.0, 0.0)
    poisoned = np.full_like(C0, np.nan)
    hip.lib.tns_set_option(TNS_OPT_STRICT_BETA0, 0)
    try:
        for v in forms(hip):
            assert_bits(run_form(hip, torch_cuda, v, A, B, poisoned, 1.0, 0.0), ref,
                        (v, M, N, K, "blas beta 0"))
    finally:
        hip.lib.tns_set_option(TNS_OPT_STRICT_BETA0, 1)


@pytest.mark.parametrize("K", [96, 128, 192])
def test_strict_beta0_specials(hip, torch_cuda, ora, K):
    """Strict beta = 0 is the reference's 0*C: NaN and Inf in C survive, and a
    negative C starts the chain from -0.  The specials sit in every
    accumulator row (rows 0, 32, 64, 96 of both 128-row halves), each row
    loaded by its own group of C loads in the row-ordered front."""
    M = N = 256
    A, B, C0 = operands(77 + K, M, N, K)
    C0 = -np.abs(C0) - np.float32(0.25)  # negative finite everywhere
    specials = [np.nan, np.inf, -np.inf, np.nan]
    for half in (0, 128):
        for i, r in enumerate((0, 32, 64, 96)):
            C0[half + r, (37 * i + half + 5) % N] = specials[i]
            C0[half + r + 7, (91 * i + half + 130) % N] = specials[(i + 1) % 4]
    ref = reference(ora, A, B, C0, 1.0, 0.0)
    assert np.isnan(ref).sum() >= 16
    for v in forms(hip):
        assert_bits(run_form(hip, torch_cuda, v, A, B, C0, 1.0, 0.0), ref, (v, K))
    # A == 0 and B < 0: every product is -0, so the chain stays at the -0 it
    # starts from (a chain started from +0 would end at +0)
    Z = np.zeros_like(A)
    Bn = -np.abs(B) - np.float32(0.5)
    ref = reference(ora, Z, Bn, C0, 1.0, 0.0)
    fin = np.isfinite(ref)
    assert np.all(ref.view(np.uint32)[fin] == 0x80000000)
    for v in forms(hip):
        assert_bits(run_form(hip, torch_cuda, v, Z, Bn, C0, 1.0, 0.0), ref, (v, K, "A = 0"))


@pytest.mark.parametrize("K", [64, 128, 160])
def test_padded_leading_dims_and_offsets(hip, torch_cuda, ora, K):
    """lda > K, ldb > N, ldc > N and non-zero element offsets (multiples of 4):
    the padding of C keeps its values."""
    M, N = 512, 256
    lda, ldb, ldc = K + 4, N + 8, N + 12
    oa, ob, oc = 4, 8, 12
    rng = np.random.default_rng(300 + K)
    A = rng.uniform(-1, 1, oa + M * lda).astype(np.float32)
    B = rng.uniform(-1, 1, ob + K * ldb).astype(np.float32)
    C = rng.uniform(-1, 1, oc + M * ldc).astype(np.float32)
    for alpha, beta in [(0.5, 2.0), (1.0, 0.0)]:
        ref = C.copy()
        ora.sgemm(False, False, M, N, K, alpha, A[oa:], lda, B[ob:], ldb, beta, ref[oc:], ldc)
        for v in forms(hip):
            dA, dB, dC = (torch_cuda.from_numpy(x.copy()).cuda() for x in (A, B, C))
            hip.gemmVariant(v, False, False, M, N, K, alpha, dA, oa, lda, 0, dB, ob, ldb, 0, beta,
                            dC, oc, ldc, 0, 1)
            hip.finish()
            assert_bits(dC.cpu().numpy(), ref, (v, K, alpha, beta))


def test_strided_batch(hip, torch_cuda, ora):
    """Batch 3 at K = 128 (blockIdx.y = batch): front and back adjacent."""
    batch, M, N, K = 3, 256, 256, 128
    rng = np.random.default_rng(9)
    A = rng.uniform(-1, 1, (batch, M, K)).astype(np.float32)
    B = rng.uniform(-1, 1, (batch, K, N)).astype(np.float32)
    C = rng.uniform(-1, 1, (batch, M, N)).astype(np.float32)
    for alpha, beta in [(1.0, 1.0), (1.0, 0.0), (-1.5, 0.25)]:
        ref = C.copy()
        ora.sgemm_batch_strided(False, False, M, N, K, alpha, A.reshape(-1), K, M * K,
                                B.reshape(-1), N, K * N, beta, ref.reshape(-1), N, M * N, batch)
        for v in forms(hip):
            dA, dB, dC = (torch_cuda.from_numpy(x.copy()).cuda() for x in (A, B, C))
            hip.gemmVariant(v, False, False, M, N, K, alpha, dA, 0, K, M * K, dB, 0, N, K * N,
                            beta, dC, 0, N, M * N, batch)
            hip.finish()
            assert_bits(dC.cpu().numpy(), ref, (v, alpha, beta))
