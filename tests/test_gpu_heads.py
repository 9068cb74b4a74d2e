"""Dropout and the elementwise loss heads on the device, bit for bit against
tests/_heads_oracle.py: every N around the 4-element group and the 256-thread
block, 16-byte aligned and one-float-offset pointers (vector and scalar
path), separate buffers and in place, src holding NaN / Inf / -0.0 /
denormals, and the TNS_ERR_ARG cases, which must leave the outputs untouched."""
import numpy as np
import pytest

import _heads_oracle as ho

pytestmark = pytest.mark.gpu

NS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 4099]
SEEDS = [0, 1234567, 0x0FFFFFFF, 0xFFFFFFFF]
PROBS = [(0.0, 1.0), (0.2, None), (0.5, 2.0), (0.999, None)]   # None: the layer's own scale
GUARD = 8          # floats after each operand that no kernel may touch
SENT = np.float32(-77.25)
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-42, -1e-45, 3.0e38, -2.5, 1.0],
                   np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def source(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-4, 4, n).astype(np.float32)
    at = rng.permutation(n)[:max(n // 3, min(n, SPECIAL.size))]
    x[at] = np.resize(SPECIAL, at.size)
    return x


def buf(T, n, off, fill=None):
    """A device operand of n floats starting `off` floats into an allocation
    (off = 1: not 16-byte aligned), followed by GUARD sentinel floats."""
    t = T.full((off + n + GUARD,), float(SENT), device="cuda")
    v = t[off:off + n]
    if fill is not None and n:
        v.copy_(T.from_numpy(np.ascontiguousarray(fill, np.float32)))
    assert n == 0 or (v.data_ptr() % 16 == 0) == (off == 0)
    return t, v


def guard_ok(t, off, n):
    g = t[off + n:].cpu().numpy()
    return np.all(g == SENT) and (off == 0 or float(t[0].item()) == float(SENT))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
def test_dropout_forward(hip, torch_cuda, seed, inplace, off):
    T = torch_cuda
    for n in NS:
        x = source(n, n + 1)
        for p, scale in PROBS:
            p32 = np.float32(p)
            sc = float(ho.dropout_scale(p32)) if scale is None else scale
            ts, src = buf(T, n, off, x)
            tr, rnd = buf(T, n, off)
            td, dst = (ts, src) if inplace else buf(T, n, off)
            hip.forwardDropout(n, src, float(p32), sc, rnd, dst, seed)
            hip.finish()
            want_rnd, want = ho.dropout_forward(seed, p32, sc, x)
            tag = (n, p, seed, inplace, off)
            assert np.array_equal(bits(rnd.cpu().numpy()), bits(want_rnd)), ("rnd", tag)
            assert np.array_equal(bits(dst.cpu().numpy()), bits(want)), ("dst", tag)
            if not inplace:
                assert np.array_equal(bits(src.cpu().numpy()), bits(x)), ("src", tag)
            assert guard_ok(tr, off, n) and guard_ok(td, off, n), ("guard", tag)
            if p == 0.0 and n:   # nothing dropped, the rnd == 0 element included
                with np.errstate(invalid="ignore", over="ignore"):
                    assert np.array_equal(bits(want), bits(x * np.float32(sc)))


def test_dropout_forward_mixed_alignment(hip, torch_cuda):
    """One misaligned operand out of three sends the call down the scalar path."""
    T, n, seed = torch_cuda, 1023, 1234567
    x = source(n, 5)
    want_rnd, want = ho.dropout_forward(seed, np.float32(0.5), 2.0, x)
    for offs in [(1, 0, 0), (0, 1, 0), (0, 0, 1)]:
        (_, src), (tr, rnd), (td, dst) = (buf(T, n, offs[0], x), buf(T, n, offs[1]),
                                          buf(T, n, offs[2]))
        hip.forwardDropout(n, src, 0.5, 2.0, rnd, dst, seed)
        hip.finish()
        assert np.array_equal(bits(rnd.cpu().numpy()), bits(want_rnd)), offs
        assert np.array_equal(bits(dst.cpu().numpy()), bits(want)), offs
        assert guard_ok(tr, offs[1], n) and guard_ok(td, offs[2], n)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("inplace", [False, True])
def test_dropout_backward(hip, torch_cuda, inplace, off):
    T = torch_cuda
    for n in NS:
        x = source(n, n + 2)
        r = ho.dropout_rnd(1234567, n)
        for p, scale in PROBS:
            p32 = np.float32(p)
            sc = float(ho.dropout_scale(p32)) if scale is None else scale
            ts, src = buf(T, n, off, x)
            _, rnd = buf(T, n, off, r)
            td, dst = (ts, src) if inplace else buf(T, n, off)
            hip.backwardDropout(n, src, float(p32), sc, rnd, dst)
            hip.finish()
            want = ho.dropout_backward(p32, sc, x, r)
            assert np.array_equal(bits(dst.cpu().numpy()), bits(want)), (n, p, inplace, off)
            assert np.array_equal(bits(rnd.cpu().numpy()), bits(r))
            assert guard_ok(td, off, n)


def finite_source(n, seed):
    """Values whose differences and squares never come out NaN (no Inf in):
    -0.0, denormals and magnitudes whose square overflows included."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-4, 4, n).astype(np.float32)
    edge = np.array([-0.0, 0.0, 1e-42, -1e-45, 3.0e38, -3.0e38, 1e-30, 2.5e19], np.float32)
    at = rng.permutation(n)[:max(n // 3, min(n, edge.size))]
    x[at] = np.resize(edge, at.size)
    return x


@pytest.mark.parametrize("off", [0, 1])
def test_cost_l2(hip, torch_cuda, off):
    T = torch_cuda
    for n in NS:
        p, t = finite_source(n, n + 3), finite_source(n, n + 4)
        (_, dp), (_, dt) = buf(T, n, off, p), buf(T, n, off, t)
        (td, dd), (te, de) = buf(T, n, off), buf(T, n, off)
        hip.costL2(n, dp, dt, dd, de)
        hip.finish()
        d, e = ho.cost_l2(p, t)
        assert not np.isnan(e).any()
        assert np.array_equal(bits(dd.cpu().numpy()), bits(d)), ("delta", n, off)
        assert np.array_equal(bits(de.cpu().numpy()), bits(e)), ("error", n, off)
        assert guard_ok(td, off, n) and guard_ok(te, off, n)


def logistic_inputs(n, seed):
    """p over [0, 1] with 0, 1, values below eps and within eps of 1; t from
    {0, 1, 0.3}."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 1, n).astype(np.float32)
    edge = np.array([0.0, 1.0, 5e-7, 1e-6, 9.9e-7, 1e-30, 1 - 5e-7, 1 - 1e-6, 1 - 6e-8, 0.5],
                    np.float32)
    at = rng.permutation(n)[:max(n // 2, min(n, edge.size))]
    p[at] = np.resize(edge, at.size)
    t = rng.choice(np.array([0.0, 1.0, 0.3], np.float32), n).astype(np.float32)
    return p, t


@pytest.mark.parametrize("off", [0, 1])
def test_cross_entropy_logistic(hip, torch_cuda, off):
    T = torch_cuda
    for n in NS:
        p, t = logistic_inputs(n, n + 5)
        (_, dp), (_, dt) = buf(T, n, off, p), buf(T, n, off, t)
        (td, dd), (te, de) = buf(T, n, off), buf(T, n, off)
        hip.crossEntropyLogistic(n, dp, dt, dd, de)
        hip.finish()
        d, e = ho.cross_entropy_logistic(p, t)
        ge = de.cpu().numpy()
        print(f"logistic n={n} off={off}: {int((bits(ge) != bits(e)).sum())} of {n} error "
              "values differ")
        assert np.array_equal(bits(dd.cpu().numpy()), bits(d)), ("delta", n, off)
        assert np.array_equal(bits(ge), bits(e)), ("error", n, off)
        assert guard_ok(td, off, n) and guard_ok(te, off, n)
    assert np.all(np.isfinite(ho.cross_entropy_logistic(*logistic_inputs(4099, 1))[1]))


def test_arg_errors_leave_the_outputs_untouched(hip, torch_cuda):
    T, L, c = torch_cuda, hip.lib, hip.ctx
    n = 64
    a = T.full((4 * n,), float(SENT), device="cuda")
    src, rnd, dst = a[:n], a[n:2 * n], a[2 * n:3 * n]
    P = lambda t, k=0: t.data_ptr() + 4 * k  # noqa: E731
    ARG = 1
    fwd, bwd = L.tns_hip_dropout_forward, L.tns_hip_dropout_backward
    cases = [
        fwd(c, -1, 1, 0.5, 2.0, P(src), P(rnd), P(dst)),            # N < 0
        fwd(c, n, -1, 0.5, 2.0, P(src), P(rnd), P(dst)),            # seed < 0
        fwd(c, n, 1 << 32, 0.5, 2.0, P(src), P(rnd), P(dst)),       # seed >= 2^32
        fwd(c, n, 1, 0.5, 2.0, None, P(rnd), P(dst)),               # null operands
        fwd(c, n, 1, 0.5, 2.0, P(src), None, P(dst)),
        fwd(c, n, 1, 0.5, 2.0, P(src), P(rnd), None),
        fwd(c, n, 1, 0.5, 2.0, P(src), P(src), P(dst)),             # rnd is src
        fwd(c, n, 1, 0.5, 2.0, P(src), P(dst, 1), P(dst)),          # rnd overlaps dst
        fwd(c, n, 1, 0.5, 2.0, P(src), P(src, n - 1), P(dst)),      # rnd overlaps src's end
        fwd(c, n, 1, 0.5, 2.0, P(src), P(a, 3 * n), P(src, 4)),     # src, dst shifted by 4
        fwd(None, n, 1, 0.5, 2.0, P(src), P(rnd), P(dst)),          # null context
        bwd(c, -1, 0.5, 2.0, P(src), P(rnd), P(dst)),
        bwd(c, n, 0.5, 2.0, None, P(rnd), P(dst)),
        bwd(c, n, 0.5, 2.0, P(src), None, P(dst)),
        bwd(c, n, 0.5, 2.0, P(src), P(rnd), None),
        bwd(c, n, 0.5, 2.0, P(src), P(dst, 1), P(dst)),
        bwd(c, n, 0.5, 2.0, P(src), P(src), P(src)),
        bwd(c, n, 0.5, 2.0, P(src), P(rnd), P(src, 1)),
    ]
    for f in (L.tns_hip_cost_l2, L.tns_hip_cross_entropy_logistic):
        cases += [f(c, -1, P(src), P(rnd), P(dst), P(a, 3 * n)),
                  f(c, n, None, P(rnd), P(dst), P(a, 3 * n)),
                  f(c, n, P(src), None, P(dst), P(a, 3 * n)),
                  f(c, n, P(src), P(rnd), None, P(a, 3 * n)),
                  f(c, n, P(src), P(rnd), P(dst), None)]
    hip.finish()
    assert cases == [ARG] * len(cases), cases
    assert bool((a == float(SENT)).all()), "a refused call wrote to an operand"
    # N == 0 is a no-op, null operands and all
    assert fwd(c, 0, 1, 0.5, 2.0, None, None, None) == 0
    assert bwd(c, 0, 0.5, 2.0, None, None, None) == 0
    assert L.tns_hip_cost_l2(c, 0, None, None, None, None) == 0
    assert L.tns_hip_cross_entropy_logistic(c, 0, None, None, None, None) == 0
    # the largest seed and the exact in-place call are accepted
    assert fwd(c, n, 0xFFFFFFFF, 0.5, 2.0, P(src), P(rnd), P(src)) == 0
    hip.finish()
    L.tns_clear_error()
