"""Oracle sanity at larger sizes: agreement with float64 numpy within the
componentwise dot-product bound used for all GEMM parity:
    |C - C64| <= tol * (|alpha| |A||B| + |beta| |C0|)_ij
plus exact small-integer known answers (any summation order is exact)."""
import numpy as np
import pytest


def ref64(ta, tb, A, B, alpha, beta, C0):
    a = A.T if ta else A
    b = B.T if tb else B
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    c = alpha * (a64 @ b64) + beta * C0.astype(np.float64)
    bound = abs(alpha) * (np.abs(a64) @ np.abs(b64)) + abs(beta) * np.abs(C0.astype(np.float64))
    return c, bound


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(37, 53, 61), (1, 97, 33), (64, 1, 129), (128, 96, 300)])
def test_gemm_vs_float64(ora, ta, tb, M, N, K):
    rng = np.random.default_rng(M * 1000 + N * 10 + K)
    A = rng.uniform(-1, 1, (K, M) if ta else (M, K)).astype(np.float32)
    B = rng.uniform(-1, 1, (N, K) if tb else (K, N)).astype(np.float32)
    C0 = rng.uniform(-1, 1, (M, N)).astype(np.float32)
    for alpha, beta in [(1.0, 0.0), (0.5, 2.0), (1.0, 1.0)]:
        C = C0.copy()
        ora.sgemm(bool(ta), bool(tb), M, N, K, alpha, A, A.shape[1], B, B.shape[1], beta, C, N)
        c64, bound = ref64(ta, tb, A, B, alpha, beta, C0)
        assert np.all(np.abs(C - c64) <= 1e-5 * bound + 1e-30)


def test_gemm_exact_integers(ora):
    rng = np.random.default_rng(7)
    M, N, K = 19, 23, 29
    A = rng.integers(-8, 8, (M, K)).astype(np.float32)
    B = rng.integers(-8, 8, (K, N)).astype(np.float32)
    exact = (A.astype(np.int64) @ B.astype(np.int64)).astype(np.float32)
    for ta, tb in [(0, 0), (0, 1), (1, 0), (1, 1)]:
        a = np.ascontiguousarray(A.T) if ta else A
        b = np.ascontiguousarray(B.T) if tb else B
        C = np.zeros((M, N), np.float32)
        ora.sgemm(bool(ta), bool(tb), M, N, K, 1.0, a, a.shape[1], b, b.shape[1], 0.0, C, N)
        assert np.array_equal(C, exact)


def test_gemm_rows_equals_full(ora):
    rng = np.random.default_rng(3)
    M, N, K = 64, 80, 96
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    B = rng.uniform(-1, 1, (K, N)).astype(np.float32)
    full = np.zeros((M, N), np.float32)
    ora.sgemm(False, False, M, N, K, 1.0, A, K, B, N, 0.0, full, N)
    part = np.zeros((M, N), np.float32)
    ora.sgemm_rows(False, False, 8, 24, M, N, K, 1.0, A, K, B, N, 0.0, part, N)
    assert np.array_equal(part[8:24], full[8:24])


def test_threads_do_not_change_results(ora):
    rng = np.random.default_rng(11)
    M, N, K = 33, 65, 130
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    B = rng.uniform(-1, 1, (K, N)).astype(np.float32)
    outs = []
    for t in (1, 2, 5, 8):
        ora.set_threads(t)
        C = np.zeros((M, N), np.float32)
        ora.sgemm(False, False, M, N, K, 1.0, A, K, B, N, 0.0, C, N)
        outs.append(C)
    ora.set_threads(0)
    for o in outs[1:]:
        assert o.tobytes() == outs[0].tobytes()


def test_im2col_1x1_identity(ora):
    x = np.arange(2 * 3 * 4, dtype=np.float32)
    col = ora.im2col(2, 3, 4, 1, 1, 0, 0, 1, 1, 1, 1, x)
    assert col.ravel().tobytes() == x.tobytes()


def test_col2im_is_adjoint_of_im2col_without_dilation(ora):
    # <im2col(x), y> == <x, col2im(y)> when dilation == 1 (the reference's
    # col2im formula only departs from the adjoint for dilation > 1)
    rng = np.random.default_rng(5)
    C, H, W, k, p, s = 3, 9, 7, 3, 1, 2
    x = rng.integers(-4, 4, C * H * W).astype(np.float32)
    col = ora.im2col(C, H, W, k, k, p, p, s, s, 1, 1, x)
    y = rng.integers(-4, 4, col.size).astype(np.float32)
    back = np.zeros(C * H * W, np.float32)
    ora.col2im(C, H, W, k, k, p, p, s, s, 1, 1, y.copy(), back)
    assert float(np.dot(col.ravel().astype(np.float64), y)) == float(np.dot(x.astype(np.float64), back))


def test_conv_forward_matches_direct(ora):
    rng = np.random.default_rng(9)
    batch, C, H, W, F, k, s, p = 2, 3, 11, 11, 5, 3, 2, 1
    x = rng.uniform(0, 1, (batch, C, H, W)).astype(np.float32)
    w = rng.uniform(-0.3, 0.3, (F, C * k * k)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, F).astype(np.float32)
    out = ora.conv_forward(x, w, b, F, k, s, p, 4)
    # direct float64 convolution
    oh = (H + 2 * p - k) // s + 1
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (p, p), (p, p)))
    ref = np.zeros((batch, F, oh, oh))
    wk = w.reshape(F, C, k, k).astype(np.float64)
    for i in range(oh):
        for j in range(oh):
            patch = xp[:, :, i * s:i * s + k, j * s:j * s + k]
            ref[:, :, i, j] = np.einsum("bckl,fckl->bf", patch, wk)
    ref += b[None, :, None, None]
    assert np.allclose(out, ref, atol=1e-5, rtol=1e-5)


def test_uniform_is_deterministic_and_in_range(ora):
    a = ora.uniform(1000, 2, 7)
    b = ora.uniform(1000, 2, 7)
    c = ora.uniform(1000, 2, 8)
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert a.min() >= -1.0 and a.max() < 1.0


# ---- non-square planes and per-axis windows against float64 ---------------
# The GPU suite compares bit for bit with the oracle, so the oracle itself is
# pinned here on the geometry those tests use: a plain float64 convolution
# (loop over taps, slice the zero-padded image with per-axis stride and
# dilation, einsum over channels) within the componentwise bound
# |got - ref| <= TOL * (|x| conv |w|), TOL as in test_gpu_sgemm.py.
TOL = 1e-4


def _odim(n, p, k, d, s):
    return (n + 2 * p - (d * (k - 1) + 1)) // s + 1


def conv64(x, w, pH, pW, sY, sX, dY, dX):
    """x (B,C,H,W), w (F,C,kH,kW) -> float64 (B,F,oh,ow)."""
    B, C, H, W = x.shape
    F, _, kH, kW = w.shape
    oh, ow = _odim(H, pH, kH, dY, sY), _odim(W, pW, kW, dX, sX)
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (pH, pH), (pW, pW)))
    w64 = w.astype(np.float64)
    out = np.zeros((B, F, oh, ow))
    for kr in range(kH):
        for kc in range(kW):
            win = xp[:, :, kr * dY:kr * dY + (oh - 1) * sY + 1:sY,
                     kc * dX:kc * dX + (ow - 1) * sX + 1:sX]
            out += np.einsum("bcij,fc->bfij", win, w64[:, :, kr, kc])
    return out


def conv64_dw(x, delta, kH, kW, pH, pW, sY, sX):
    """sum over images and pixels of delta[b,f,i,j] * x window -> (F,C,kH,kW)."""
    B, C, H, W = x.shape
    F, oh, ow = delta.shape[1:]
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (pH, pH), (pW, pW)))
    d64 = delta.astype(np.float64)
    dw = np.zeros((F, C, kH, kW))
    for kr in range(kH):
        for kc in range(kW):
            win = xp[:, :, kr:kr + (oh - 1) * sY + 1:sY, kc:kc + (ow - 1) * sX + 1:sX]
            dw[:, :, kr, kc] = np.einsum("bfij,bcij->fc", d64, win)
    return dw


def conv64_dx(w, delta, H, W, pH, pW, sY, sX):
    """the adjoint of conv64 in x (dilation 1) -> (B,C,H,W)."""
    F, C, kH, kW = w.shape
    B, _, oh, ow = delta.shape
    gp = np.zeros((B, C, H + 2 * pH, W + 2 * pW))
    w64, d64 = w.astype(np.float64), delta.astype(np.float64)
    for kr in range(kH):
        for kc in range(kW):
            gp[:, :, kr:kr + (oh - 1) * sY + 1:sY, kc:kc + (ow - 1) * sX + 1:sX] += \
                np.einsum("bfij,fc->bcij", d64, w64[:, :, kr, kc])
    return gp[:, :, pH:pH + H, pW:pW + W]


NONSQUARE_CONV = [  # B, C, H, W, F, k, s, p, d
    (2, 3, 9, 14, 5, 3, 1, 1, 1), (2, 4, 14, 9, 6, 3, 2, 1, 1), (1, 5, 7, 20, 4, 1, 1, 0, 1),
    (2, 3, 12, 17, 4, 3, 1, 2, 2), (1, 2, 6, 11, 3, 5, 2, 2, 1)]
ANISO_IM2COL = [  # C, H, W, kH, kW, pH, pW, sY, sX, dY, dX
    (3, 9, 14, 3, 2, 1, 0, 1, 2, 1, 1), (2, 11, 8, 1, 3, 0, 2, 2, 1, 1, 2),
    (2, 10, 13, 2, 3, 1, 1, 3, 1, 2, 1), (1, 7, 16, 3, 1, 0, 0, 1, 3, 2, 1)]
NONSQUARE_BACKWARD = [  # B, C, H, W, F, k, s, p
    (2, 3, 9, 14, 5, 3, 1, 1), (2, 4, 14, 9, 6, 3, 2, 1)]

for _B, _C, _H, _W, _F, _k, _s, _p, _d in NONSQUARE_CONV:
    assert _H != _W and _odim(_H, _p, _k, _d, _s) != _odim(_W, _p, _k, _d, _s)
    assert _s != 2 or _H % 2 != _W % 2
for _C, _H, _W, _kH, _kW, _pH, _pW, _sY, _sX, _dY, _dX in ANISO_IM2COL:
    assert _H != _W and _odim(_H, _pH, _kH, _dY, _sY) != _odim(_W, _pW, _kW, _dX, _sX)
for _B, _C, _H, _W, _F, _k, _s, _p in NONSQUARE_BACKWARD:
    assert _H != _W and _odim(_H, _p, _k, 1, _s) != _odim(_W, _p, _k, 1, _s)
    assert _s != 2 or _H % 2 != _W % 2


@pytest.mark.parametrize("B,C,H,W,F,k,s,p,d", NONSQUARE_CONV)
def test_conv_forward_nonsquare_vs_float64(ora, B, C, H, W, F, k, s, p, d):
    rng = np.random.default_rng(H * 100 + W)
    x = rng.uniform(-1, 1, (B, C, H, W)).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (F, C, k, k)).astype(np.float32)
    got = ora.conv_forward(x, w.ravel(), np.zeros(F, np.float32), F, k, s, p, 4, d)
    ref = conv64(x, w, p, p, s, s, d, d)
    bound = conv64(np.abs(x), np.abs(w), p, p, s, s, d, d)
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= TOL * bound + 1e-30)


@pytest.mark.parametrize("geo", ANISO_IM2COL)
def test_im2col_per_axis_vs_float64(ora, geo):
    C, H, W, kH, kW, pH, pW, sY, sX, dY, dX = geo
    rng = np.random.default_rng(sum(geo))
    F = 3
    x = rng.uniform(-1, 1, (1, C, H, W)).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (F, C, kH, kW)).astype(np.float32)
    col = ora.im2col(*geo, x.ravel())[0]
    oh, ow = _odim(H, pH, kH, dY, sY), _odim(W, pW, kW, dX, sX)
    assert col.shape == (C * kH * kW, oh * ow) and not np.isnan(col).any()
    got = (w.reshape(F, -1).astype(np.float64) @ col.astype(np.float64)).reshape(1, F, oh, ow)
    ref = conv64(x, w, pH, pW, sY, sX, dY, dX)
    bound = conv64(np.abs(x), np.abs(w), pH, pW, sY, sX, dY, dX)
    assert np.all(np.abs(got - ref) <= TOL * bound + 1e-30)


@pytest.mark.parametrize("geo", [g for g in ANISO_IM2COL if g[9:] == (1, 1)] + [
    (C, H, W, k, k, p, p, s, s, 1, 1) for _, C, H, W, _, k, s, p, d in NONSQUARE_CONV if d == 1])
def test_col2im_adjoint_identity_nonsquare(ora, geo):
    # integers: both inner products are exact in any order
    C, H, W = geo[:3]
    rng = np.random.default_rng(sum(geo) + 1)
    x = rng.integers(-4, 4, C * H * W).astype(np.float32)
    col = ora.im2col(*geo, x)
    g = rng.integers(-4, 4, col.size).astype(np.float32)
    back = np.zeros(C * H * W, np.float32)
    ora.col2im(*geo, g.copy(), back)
    assert float(np.dot(col.ravel().astype(np.float64), g)) == \
        float(np.dot(x.astype(np.float64), back))


@pytest.mark.parametrize("B,C,H,W,F,k,s,p", NONSQUARE_BACKWARD)
def test_conv_backward_nonsquare_vs_float64(ora, B, C, H, W, F, k, s, p):
    rng = np.random.default_rng(H * 100 + W + 7)
    oh, ow = _odim(H, p, k, 1, s), _odim(W, p, k, 1, s)
    x = rng.uniform(-1, 1, (B, C, H, W)).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (F, C, k, k)).astype(np.float32)
    out = rng.uniform(-1, 1, (B, F, oh, ow)).astype(np.float32)
    delta = rng.uniform(-1, 1, out.shape).astype(np.float32)
    wu0 = rng.uniform(-1, 1, w.size).astype(np.float32)
    sd0 = rng.uniform(-1, 1, x.shape).astype(np.float32)
    d, bu, wu, sd = delta.copy(), np.zeros(F, np.float32), wu0.copy(), sd0.copy()
    ora.conv_backward(x, w.ravel(), F, k, s, p, 4, out, d, bu, wu, sd)   # linear: delta kept
    assert np.array_equal(d, delta)
    ref = wu0.astype(np.float64) + conv64_dw(x, delta, k, k, p, p, s, s).ravel()
    bound = np.abs(wu0) + conv64_dw(np.abs(x), np.abs(delta), k, k, p, p, s, s).ravel()
    assert np.all(np.abs(wu - ref) <= TOL * bound + 1e-30)
    ref = sd0.astype(np.float64) + conv64_dx(w, delta, H, W, p, p, s, s)
    bound = np.abs(sd0) + conv64_dx(np.abs(w), np.abs(delta), H, W, p, p, s, s)
    assert np.all(np.abs(sd - ref) <= TOL * bound + 1e-30)


def test_conv2d_per_axis_vs_float64_and_unequal_dilation_refused(ora):
    """oracle.conv2d with the eight per-axis parameters (Conv2D's order: w
    before h, x before y); unequal dilations whose swapped im2col grid differs
    from the output's raise before the oracle can pass its workspace."""
    rng = np.random.default_rng(31)
    B, C, H, W, F, kH, kW, wP, hP, xS, yS, dil = 2, 6, 15, 10, 9, 3, 2, 0, 1, 2, 1, 1
    x = rng.uniform(-1, 1, (B, C, H, W)).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, (F, C, kH, kW)).astype(np.float32)
    got = ora.conv2d(x, w.ravel(), F, kH=kH, kW=kW, wPad=wP, hPad=hP, xStride=xS, yStride=yS,
                     dil=dil)
    ref = conv64(x, w, hP, wP, yS, xS, dil, dil)
    bound = conv64(np.abs(x), np.abs(w), hP, wP, yS, xS, dil, dil)
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= TOL * bound + 1e-30)
    # negative paddings: dilation + k div 2 - 1 (ntensors.pas:8266-8269)
    got = ora.conv2d(x, w.ravel(), F, kH=kH, kW=kW, pad=-1, stride=1, dil=2)
    assert np.array_equal(got, ora.conv2d(x, w.ravel(), F, kH=kH, kW=kW, wPad=2 + kW // 2 - 1,
                                          hPad=2 + kH // 2 - 1, stride=1, dil=2))
    x = rng.uniform(-1, 1, (1, 2, 12, 20)).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, 3 * 2 * 9).astype(np.float32)
    for xd, yd, xx in ((1, 2, x), (2, 1, x), (1, 2, x[:, :, :, :12].copy())):
        with pytest.raises(ValueError, match="im2col grid"):
            ora.conv2d(xx, w, 3, 3, 0, 1, xDil=xd, yDil=yd)
    # the C entry refuses on its own too, leaving out untouched
    out = np.full((1, 3, 8, 18), 7.0, np.float32)
    ws = np.zeros(2 * 9 * 10 * 18, np.float32)
    rc = ora.lib().ora_conv2d(1, 2, 12, 20, x.ctypes.data, w.ctypes.data, 3, 3, 3, 0, 0, 1, 1, 1,
                              2, ws.ctypes.data, out.ctypes.data)
    assert rc == -1 and np.all(out == 7.0) and not ws.any()
