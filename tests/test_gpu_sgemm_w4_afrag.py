"""The fragment reads of the one-wave-per-SIMD large-NN SGEMM (sgemm_nn_w4.hip),
forced through gemmVariant by name: the picked form and the flat form, whose
regular k-loop reads its fragments from addresses held in registers (two tiles
an iteration, one per LDS stage, and an odd last one), and the form that keeps
the per-step address arithmetic.  All three run the reference's ascending-k
fma chain from beta*C per element, so every case is compared with the oracle
bit for bit: NaNs in the same places and the same uint32 words wherever the
reference is finite.

Shapes are one block and two (256 x 256, 512 x 256); K = 32 .. 192 gives the
flat fallback below four k-tiles (one tile, and a pair), front and back
adjacent at four (no regular tile), and one and two regular tiles at five and
six (the flat form's loop: pairs of tiles and an odd last one).  The picked
form takes the register-held addresses from eight k-tiles on, so K = 256 and
288 are there too: its loop runs two pairs, and two pairs and an odd tile.
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PICKED = "256x256x32_w2x2_dma_nn_big"
FLAT = "256x256x32_w2x2_dma_flat_nn_big"
B32 = "256x256x32_w2x2_dma_b32_nn_big"
SHAPES = [(256, 256), (512, 256)]


def forms(hip):
    names = hip.gemmVariants()
    return [names.index(PICKED), names.index(FLAT), names.index(B32)]


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


# (K, k-tile that holds the witness): the first tile at one and four k-tiles,
# and regular tiles of the picked form's loop at nine: both stages of a pair
# and the odd last one
@pytest.mark.parametrize("K,tile", [(32, 0), (128, 0), (288, 2), (288, 3), (288, 6)])
@pytest.mark.parametrize("M,N", SHAPES)
def test_order_witness(hip, torch_cuda, ora, M, N, K, tile):
    """A step that is handed the wrong k changes the result of whole rows, on
    every column.  B is all ones, C = 0 under strict beta = 0, alpha = 1; row m
    of A is zero except three k inside one 4-k group of one k-tile: 2^24
    at k1, -2^24 at k2, 1 at k3, the rows running through all 24 arrangements
    of all 8 groups (192 of every 256 rows).  In the ascending chain the 1 is
    lost exactly when it meets +2^24 (1 + 2^24 and 2^24 + 1 round to 2^24),
    that is when k1 < k2 and k3 < k2: those rows end at 0, the others at 1
    (1 - 2^24 is exact).  The arithmetic is exact, so the oracle's result is
    asserted to hold both values and nothing else."""
    A = np.zeros((M, K), np.float32)
    arr = [(g, p) for g in range(8) for p in itertools.permutations(range(4), 3)]
    for m in range(M):
        if m % 256 < len(arr):
            g, (k1, k2, k3) = arr[m % 256]
            A[m, 32 * tile + 4 * g + k1] = 2.0 ** 24
            A[m, 32 * tile + 4 * g + k2] = -(2.0 ** 24)
            A[m, 32 * tile + 4 * g + k3] = 1.0
    B = np.ones((K, N), np.float32)
    C0 = np.zeros((M, N), np.float32)
    ref = reference(ora, A, B, C0, 1.0, 0.0)
    want = np.zeros(M, np.float32)
    for m in range(M):
        if m % 256 < len(arr):
            _, (k1, k2, k3) = arr[m % 256]
            want[m] = 0.0 if (k1 < k2 and k3 < k2) else 1.0
    assert np.array_equal(ref, np.repeat(want[:, None], N, axis=1))
    assert (ref == 1.0).any() and (ref[: len(arr)] == 0.0).any()
    for v in forms(hip):
        assert_bits(run_form(hip, torch_cuda, v, A, B, C0, 1.0, 0.0), ref, (v, M, N, K, tile))


@pytest.mark.parametrize("K", [32, 64, 128, 160, 192, 256, 288])
@pytest.mark.parametrize("M,N", SHAPES)
def test_row_and_tile_coverage(hip, torch_cuda, ora, M, N, K):
    """Uniform random operands, one to nine k-tiles, alpha = 1 on beta = 0 and
    1, and a scaled mode (A_PART = ALPHA*A rounded once, after the read)."""
    rng = np.random.default_rng(7000 * M + K)
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    B = rng.uniform(-1, 1, (K, N)).astype(np.float32)
    C0 = rng.uniform(-1, 1, (M, N)).astype(np.float32)
    for alpha, beta in [(1.0, 0.0), (1.0, 1.0), (-1.5, 0.25)]:
        ref = reference(ora, A, B, C0, alpha, beta)
        for v in forms(hip):
            assert_bits(run_form(hip, torch_cuda, v, A, B, C0, alpha, beta), ref,
                        (v, M, N, K, alpha, beta))


@pytest.mark.parametrize("K", [64, 160])
def test_padded_lda_and_offsets(hip, torch_cuda, ora, K):
    """lda = K + 4 and element offsets that are multiples of 4 (the DMA's
    16-byte alignment) on all three operands."""
    M, N = 512, 256
    lda, oa, ob, oc = K + 4, 4, 8, 12
    rng = np.random.default_rng(500 + K)
    A = rng.uniform(-1, 1, oa + M * lda).astype(np.float32)
    B = rng.uniform(-1, 1, ob + K * N).astype(np.float32)
    C = rng.uniform(-1, 1, oc + M * N).astype(np.float32)
    for alpha, beta in [(1.0, 1.0), (-1.5, 0.25)]:
        ref = C.copy()
        ora.sgemm(False, False, M, N, K, alpha, A[oa:], lda, B[ob:], N, beta, ref[oc:], N)
        for v in forms(hip):
            dA, dB, dC = (torch_cuda.from_numpy(x.copy()).cuda() for x in (A, B, C))
            hip.gemmVariant(v, False, False, M, N, K, alpha, dA, oa, lda, 0, dB, ob, N, 0, beta,
                            dC, oc, N, 0, 1)
            hip.finish()
            assert_bits(dC.cpu().numpy(), ref, (v, K, alpha, beta))


def test_strided_batch(hip, torch_cuda, ora):
    """Strided batch of 3 at K = 128."""
    batch, M, N, K = 3, 256, 256, 128
    rng = np.random.default_rng(19)
    A = rng.uniform(-1, 1, (batch, M, K)).astype(np.float32)
    B = rng.uniform(-1, 1, (batch, K, N)).astype(np.float32)
    C = rng.uniform(-1, 1, (batch, M, N)).astype(np.float32)
    for alpha, beta in [(1.0, 0.0), (-1.5, 0.25)]:
        ref = C.copy()
        ora.sgemm_batch_strided(False, False, M, N, K, alpha, A.reshape(-1), K, M * K,
                                B.reshape(-1), N, K * N, beta, ref.reshape(-1), N, M * N, batch)
        for v in forms(hip):
            dA, dB, dC = (torch_cuda.from_numpy(x.copy()).cuda() for x in (A, B, C))
            hip.gemmVariant(v, False, False, M, N, K, alpha, dA, 0, K, M * K, dB, 0, N, K * N,
                            beta, dC, 0, N, M * N, batch)
            hip.finish()
            assert_bits(dC.cpu().numpy(), ref, (v, alpha, beta))
