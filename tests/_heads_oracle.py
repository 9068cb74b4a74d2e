"""numpy restatement of dropout and the elementwise loss heads, written from
the reference's text:

* forward_dropout / backward_dropout / cost_l2: the device kernels
  (cuda_sgemm.cu:1617-1662).  rand_xorshift(seed + i) is one xorshift64* step
  in unsigned 64-bit arithmetic, `% RANDOM_MAX` keeps 28 bits, the store to
  the float rnd[i] rounds to nearest even and `/= RANDOM_MAX` is exact.
* logisticCrossEntropy: the CPU loop (nlogisticlayer.pas:67-78): t, p single;
  max(p, eps), 1 - p and 1 - t in single, ln returns double, so the products
  and the subtraction are double and the store rounds once.
"""
import numpy as np

RANDOM_MAX = 0x10000000
SEPS = np.float32(0.000001)   # sEPSILON, ntensors.pas:95
_MASK = (1 << 64) - 1


def xorshift_r(seed: int, i: int) -> int:
    """rand_xorshift(seed + i) as a Python integer (exact)."""
    assert 0 <= seed < 1 << 32
    x = (seed + i) & _MASK
    x ^= x >> 12
    x ^= (x << 25) & _MASK
    x ^= x >> 27
    x = (x * 0x2545F4914F6CDD1D) & _MASK
    return x % RANDOM_MAX


def dropout_r(seed: int, n: int, start: int = 0) -> np.ndarray:
    """r for elements start .. start + n - 1 (uint64 array)."""
    assert 0 <= seed < 1 << 32
    x = np.uint64(seed) + np.arange(start, start + n, dtype=np.uint64)
    x ^= x >> np.uint64(12)
    x ^= x << np.uint64(25)
    x ^= x >> np.uint64(27)
    with np.errstate(over="ignore"):
        x = x * np.uint64(0x2545F4914F6CDD1D)
    return x % np.uint64(RANDOM_MAX)


def dropout_rnd(seed: int, n: int, start: int = 0) -> np.ndarray:
    r = dropout_r(seed, n, start).astype(np.float32)      # nearest even
    return r / np.float32(RANDOM_MAX)                     # exact


def _select(rnd, probability, src, scale):
    with np.errstate(invalid="ignore", over="ignore"):
        kept = (src.astype(np.float32) * np.float32(scale)).astype(np.float32)
    return np.where(rnd < np.float32(probability), np.float32(0.0), kept).astype(np.float32)


def dropout_forward(seed, probability, scale, src):
    """-> (rnd, dst)"""
    rnd = dropout_rnd(seed, src.size)
    return rnd, _select(rnd, probability, src, scale)


def dropout_backward(probability, scale, src, rnd):
    return _select(rnd, probability, src, scale)


def dropout_scale(probability) -> np.float32:
    """TDropoutLayer.Create: scale := 1 / (1.0 - probability), probability a
    single, the expression double, the field single."""
    return np.float32(1.0 / (1.0 - float(np.float32(probability))))


def cost_l2(pred, truth):
    """-> (delta, error)"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = (truth.astype(np.float32) - pred.astype(np.float32)).astype(np.float32)
        return r, (r * r).astype(np.float32)


def cross_entropy_logistic(pred, truth):
    """-> (delta, error)"""
    p, t = pred.astype(np.float32), truth.astype(np.float32)
    a = np.where(p > SEPS, p, SEPS).astype(np.float32)          # math.max: a > b ? a : b
    q = (np.float32(1) - p).astype(np.float32)
    b = np.where(q > SEPS, q, SEPS).astype(np.float32)
    u = (np.float32(1) - t).astype(np.float32)
    e = (-t).astype(np.float64) * np.log(a.astype(np.float64)) \
        - u.astype(np.float64) * np.log(b.astype(np.float64))
    return (t - p).astype(np.float32), e.astype(np.float32)
