"""CPU check of oracle.softmax_batch (the (batch, group) loop of
TSoftmaxLayer.softmaxBatch over ora_softmax, nsoftmaxlayer.pas:83-121) against
a float64 numpy softmax, at the grouped / strided / offset cases the GPU test
of tns_hip_softmax_batch replays (tests/test_gpu_train.py imports them)."""
import numpy as np
import pytest

# (n, batch, batch_size, groups, group_size, stride, temp, offset)
SOFTMAX_CASES = [
    (5, 6, 23, 4, 5, 1, 1.0, 0),      # [softmax] groups = 4; 3 elements of row padding
    (5, 3, 70, 4, 16, 3, 1.0, 0),     # stride 3 inside each group's 16 elements
    (6, 3, 24, 4, 1, 4, 1.0, 0),      # channel softmax: the groups interleave (stride = groups)
    (5, 6, 23, 4, 5, 1, 0.5, 0),      # temperatures
    (5, 6, 23, 4, 5, 1, 2.0, 0),
    (5, 3, 70, 4, 16, 3, 1.0 / 3.0, 2),
    (7, 5, 40, 1, 0, 1, 1.0, 9),      # softmax-tree group: iOffset = oOffset = count
    (10, 256, 10, 1, 0, 1, 1.0, 0),   # batch * groups: one full block of threads
    (3, 257, 3, 1, 0, 1, 1.0, 0),     # one thread into the second block
    (4, 250, 16, 4, 4, 1, 1.0, 1),    # 1000 rows
    (1, 4, 3, 2, 1, 1, 1.0, 0),       # n = 1
    (0, 4, 8, 2, 4, 1, 1.0, 0),       # n = 0: nothing is written
]
TAIL = 11  # elements past the last row, which stay untouched


def softmax_positions(n, batch, batch_size, groups, group_size, stride):
    """Element index (from the offset) of every softmax input, [b, g, i]."""
    b, g, i = np.meshgrid(np.arange(batch), np.arange(groups), np.arange(n), indexing="ij")
    return b * batch_size + g * group_size + i * stride


def softmax_input(ora, case, seed=41):
    n, batch, batch_size, groups, group_size, stride, temp, off = case
    ext = (batch - 1) * batch_size + (groups - 1) * max(group_size, 0) + max(n - 1, 0) * stride + 1
    return ora.uniform(off + ext + TAIL, seed, n + batch, -5.0, 5.0)


def tiny_exp_input():
    """One row whose exponentials (x - max in the comment) are normal,
    subnormal (float's least normal is exp(-87.3), least subnormal exp(-103.3))
    and exactly 0."""
    return np.array([-3.0, 0.0, -95.0, -97.5, -100.0, -103.0, -104.5, -110.0, -200.0, -88.0],
                    np.float32) + np.float32(1.5)


@pytest.mark.parametrize("case", SOFTMAX_CASES)
def test_softmax_batch_vs_float64(ora, case):
    n, batch, batch_size, groups, group_size, stride, temp, off = case
    x = softmax_input(ora, case)
    keep = x.copy()
    got = ora.softmax_batch(x[off:], n, batch, batch_size, groups, group_size, stride,
                            np.float32(temp))
    assert np.array_equal(x, keep), "the input was modified"
    idx = softmax_positions(n, batch, batch_size, groups, group_size, stride)
    touched = np.zeros(got.size, bool)
    touched[idx.ravel()] = True
    assert touched.sum() == idx.size, "the case's groups overlap"
    assert np.array_equal(got[~touched], x[off:][~touched]), "wrote between / past the rows"
    if n == 0:
        return
    v = x[off:][idx].astype(np.float64)                      # [batch, groups, n]
    e = np.exp((v - v.max(axis=2, keepdims=True)) / np.float64(np.float32(temp)))
    ref = e / e.sum(axis=2, keepdims=True)
    assert np.allclose(got[idx], ref, rtol=1e-6, atol=1e-7)


def test_softmax_batch_tiny_exponentials(ora):
    x = tiny_exp_input()
    got = ora.softmax_batch(x, x.size, 1, x.size, 1, 0, 1, np.float32(1.0))
    v = x.astype(np.float64)
    e = np.exp(v - v.max())
    ref = e / e.sum()
    assert np.allclose(got, ref, rtol=1e-6, atol=1e-7)
    tiny = np.finfo(np.float32).tiny
    assert np.any((got > 0) & (got < tiny)), "no subnormal output"
    assert np.count_nonzero(got == 0) >= 3, "no exponential rounded to 0"
