"""Bias / activation / BLAS-1 kernels vs the oracle.
Bar: bit-exact for every supported activation.  logistic / tanh follow the
scalar Pascal forms with exp's real result rounded where the Pascal stores it
(tanh: two single exps, NaN once exp overflows); the device and the oracle
share that form, so only a last-ulp difference between the two libms' double
exp could separate them (not seen)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXACT = [1, 4, 8, 9, 13]
TRANSC = [0, 6]


@pytest.mark.parametrize("act", EXACT + TRANSC)
@pytest.mark.parametrize("n", [1, 7, 1024, 100003])
def test_activate(hip, torch_cuda, ora, act, n):
    x = ora.uniform(n, 8, act, -6.0, 6.0)
    if n > 100:  # overflow / underflow / signed zero edges
        x[:8] = np.array([-100, 100, 0.0, -0.0, 88.8, -88.8, 1e-8, -1e-30], np.float32)
    ref = ora.activate(x.copy(), act)
    dx = torch_cuda.from_numpy(x).cuda()
    hip.ActivateArray(n, dx, 0, act)
    hip.finish()
    got = dx.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)) or \
        np.array_equal(got, ref, equal_nan=True), (act, np.abs(got - ref).max())


@pytest.mark.parametrize("n", [5001, 5004])  # scalar and float4 forms
@pytest.mark.parametrize("act", EXACT + TRANSC)
def test_derive(hip, torch_cuda, ora, act, n):
    y = ora.activate(ora.uniform(n, 9, act, -3.0, 3.0), act)
    delta = ora.uniform(n, 10, act)
    ref = ora.gradient(y, act, delta.copy())
    dy, dd = torch_cuda.from_numpy(y).cuda(), torch_cuda.from_numpy(delta.copy()).cuda()
    hip.DeriveArray(n, dy, 0, act, dd)
    hip.finish()
    assert np.array_equal(dd.cpu().numpy(), ref)


@pytest.mark.parametrize("F,bs,batch", [(3, 5, 2), (64, 2704, 2), (255, 169, 1), (10, 1, 32),
                                        (32, 173056, 1)])
def test_forward_bias(hip, torch_cuda, ora, F, bs, batch):
    x = ora.uniform(batch * F * bs, 11, F)
    b = ora.uniform(F, 12, F, -0.1, 0.1)
    ref = ora.add_bias(x.copy(), b, F, bs, batch)
    dx, db = torch_cuda.from_numpy(x).cuda(), torch_cuda.from_numpy(b).cuda()
    hip.forwardBias(x.size, dx, 0, F, db, 1, batch)
    hip.finish()
    assert np.array_equal(dx.cpu().numpy(), ref)


@pytest.mark.parametrize("F,bs,batch", [(16, 333, 4), (3, 8, 2), (5, 7, 3), (1, 1000, 40),
                                         (4, 64, 1100), (2, 43264, 8), (3, 2053, 11),
                                         (2, 4096, 3)])
def test_backward_bias_addsums_order(hip, torch_cuda, ora, F, bs, batch):
    """addSums (ntensors.pas:7729-7781): vssum_avx2 per contiguous block,
    blocks summed in order — bit-exact.  With incb = 1 the blocks of 64 and
    more elements ((16, 333, 4), (1, 1000, 40), (4, 64, 1100), (2, 43264, 8),
    (3, 2053, 11), (2, 4096, 3)) take the lane-chain kernels of batchnorm.hip;
    (3, 8, 2) and (5, 7, 3) take backward_bias_kernel, one LDS chunk each.
    That kernel at incb != 1, at longer blocks and past one chunk:
    test_backward_bias_plain_kernel below."""
    src = ora.uniform(batch * F * bs, 13, 0)
    dst = ora.uniform(F, 14, 0)
    ref = ora.add_sums(dst.copy(), src, batch, F, bs)
    dsrc, ddst = torch_cuda.from_numpy(src).cuda(), torch_cuda.from_numpy(dst.copy()).cuda()
    hip.backwardBias(F, ddst, src.size, dsrc, 0, 1, batch)
    hip.finish()
    assert np.array_equal(ddst.cpu().numpy(), ref)
    scale = np.abs(src.reshape(batch, F, bs)).sum(axis=(0, 2)) + np.abs(dst)
    f64 = dst.astype(np.float64) + src.reshape(batch, F, bs).astype(np.float64).sum(axis=(0, 2))
    assert np.all(np.abs(ref - f64) <= 1e-5 * scale)


def test_blas1(hip, torch_cuda, ora):
    n = 10007
    x = ora.uniform(n, 15, 0)
    y = ora.uniform(n, 16, 0)
    dx, dy = torch_cuda.from_numpy(x).cuda(), torch_cuda.from_numpy(y.copy()).cuda()
    hip.axpy(n, 0.37, dx, 0, 1, dy, 0, 1)
    hip.finish()
    ref = y.copy()
    ora.lib().ora_saxpy(n, 0.37, x.ctypes.data, ref.ctypes.data)
    assert np.array_equal(dy.cpu().numpy(), ref)
    hip.scale(n, 2.5, dy, 1)
    hip.finish()
    assert np.array_equal(dy.cpu().numpy(), (ref * np.float32(2.5)).astype(np.float32))
    hip.fill(n, dy, 0, 3.0, 1)
    hip.clamp(n, 1.0, dx, dx, 1, 0)
    hip.copy(n // 2, dx, 0, 2, dy, 0, 1)
    hip.finish()
    got = dy.cpu().numpy()
    assert np.array_equal(got[: n // 2], np.clip(x, -1, 1)[0:2 * (n // 2):2])
    assert np.all(got[n // 2:] == 3.0)


def test_tnncuda_vector_ops(hip, torch_cuda):
    """TNNCuda addvv / subvv / mulvv / fmavv / fmavss / inverseSqrt
    (nncuda.pas:120-151): strided, offsets in elements, one rounding per
    arithmetic operation (numpy float32 arithmetic is the same IEEE op)."""
    T = torch_cuda
    rng = np.random.default_rng(9)
    n = 1000
    a = rng.uniform(-2, 2, 3 * n + 5).astype(np.float32)
    b = rng.uniform(-2, 2, 2 * n + 3).astype(np.float32)
    c = rng.uniform(-2, 2, n + 7).astype(np.float32)
    da, db, dc = (T.from_numpy(x).cuda() for x in (a, b, c))
    A, B, Cc = a[5::3][:n], b[3::2][:n], c[7:][:n]
    for name, ref in (("addvv", A + B), ("subvv", A - B), ("mulvv", A * B)):
        out = T.zeros(2 * n + 1, device="cuda")
        getattr(hip, name)(n, da, 5, 3, db, 3, 2, out, 1, 2)
        hip.finish()
        assert np.array_equal(out.cpu().numpy()[1::2][:n], ref.astype(np.float32)), name
    out = T.zeros(n, device="cuda")
    hip.fmavv(n, da, 5, 3, db, 3, 2, dc, 7, 1, out, 0, 1)
    hip.finish()
    assert np.array_equal(out.cpu().numpy(), ((A * B).astype(np.float32) + Cc).astype(np.float32))
    out = T.zeros(c.size, device="cuda")
    hip.fmavss(n, dc, 7, 1.5, -0.25, out)
    hip.finish()
    ref = ((Cc * np.float32(1.5)).astype(np.float32) + np.float32(-0.25)).astype(np.float32)
    assert np.array_equal(out.cpu().numpy()[7:7 + n], ref)
    v = np.abs(rng.uniform(-1e-5, 4, 2 * n)).astype(np.float32)
    v[::50] = 0.0
    dv, out = T.from_numpy(v).cuda(), T.zeros(2 * n, device="cuda")
    hip.inverseSqrt(n, 0.0, dv, out, 2, 1)
    hip.finish()
    ref = (np.float32(1) / np.sqrt(np.maximum(v[1::2], np.float32(1e-6)))).astype(np.float32)
    assert np.array_equal(out.cpu().numpy()[1::2], ref)


VV_INCS = (-2, -1, 0, 1, 3)


@pytest.mark.parametrize("n", [1, 7, 257])
@pytest.mark.parametrize("name", ["addvv", "subvv", "mulvv", "fmavv"])
def test_vector_ops_negative_and_zero_increments(hip, torch_cuda, name, n):
    """addvv / subvv / mulvv / fmavv with an increment of -2, -1, 0, 1 or 3 on
    each operand in turn (the others at 1), bit for bit NumPy's: element i of
    an operand is at i*inc from the pointer + offset, as the reference's
    kernels index it (nncuda.pas:897-950 pass the increments through as they
    come).  A negative increment walks downward, so the offset names the
    operand's last stored element and every index stays inside the buffer; 0
    reads one element n times.  dst with increment 0 is one element written n
    times: the sources then have increment 0 too, so that every write is the
    same value whatever the order.  Nothing outside the n elements is
    written."""
    T = torch_cuda
    rng = np.random.default_rng(n)
    nsrc = 3 if name == "fmavv" else 2
    G = 8                                    # sentinels on either side
    f32 = np.float32

    def operand(inc, fill):
        span = (n - 1) * abs(inc) + 1
        h = np.full(span + 2 * G, SENT, f32)
        if fill:
            h[G:G + span] = rng.uniform(-2, 2, span).astype(f32)
        off = G + (span - 1 if inc < 0 else 0)
        return h, off, off + np.arange(n) * inc       # buffer, offset, element indices

    for which in range(nsrc + 1):
        for inc in VV_INCS:
            incs = [1] * (nsrc + 1)
            incs[which] = inc
            if which == nsrc and inc == 0:
                incs = [0] * (nsrc + 1)
            srcs = [operand(i, True) for i in incs[:nsrc]]
            dh, doff, didx = operand(incs[nsrc], False)
            assert all(0 <= ix.min() and ix.max() < h.size for h, _, ix in srcs + [(dh, doff, didx)])
            v = [h[ix] for h, _, ix in srcs]
            r = {"addvv": lambda: v[0] + v[1], "subvv": lambda: v[0] - v[1],
                 "mulvv": lambda: v[0] * v[1],
                 "fmavv": lambda: (v[0] * v[1]).astype(f32) + v[2]}[name]().astype(f32)
            want = dh.copy()
            for i in range(n):
                want[didx[i]] = r[i]
            dev_srcs = [T.from_numpy(h).cuda() for h, _, _ in srcs]
            out = T.from_numpy(dh).cuda()
            args = [n]
            for d, (_, off, _), i in zip(dev_srcs, srcs, incs):
                args += [d, off, i]
            getattr(hip, name)(*args, out, doff, incs[nsrc])
            hip.finish()
            assert same(out.cpu().numpy(), want), (name, n, which, inc)


# ---- dispatch branches, grid-stride trips, alignment and increments ----------
ALL_ACTS = EXACT + TRANSC
G = 16384 * 256          # grid cap (grid_for / blocks_for) x block size
N1 = G + 259             # odd: scalar forms; the second trip spans two blocks
N4 = 4 * N1              # float4 forms at the same number of work items
SENT = np.float32(-77.25)


def same(got, ref):
    """Bit-identical, NaNs matching NaNs of any payload."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]))


def guarded(T, a, off, tail=5):
    """Device buffer [off sentinels | a | tail sentinels], 16-byte aligned."""
    h = np.concatenate([np.full(off, SENT, np.float32), np.ravel(a),
                        np.full(tail, SENT, np.float32)])
    d = T.from_numpy(h).cuda()
    assert d.data_ptr() % 16 == 0
    return d


def unguard(d, off, n):
    h = d.cpu().numpy()
    assert np.all(h[:off] == SENT) and np.all(h[off + n:] == SENT), "wrote outside the operand"
    return h[off:off + n]


@pytest.fixture(scope="module")
def big(ora):
    """Two read-only random vectors of N4 elements shared by the large cases."""
    a, b = ora.uniform(N4, 71, 0, -2.0, 2.0), ora.uniform(N4, 72, 0, -2.0, 2.0)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _backward_bias_case(hip, T, ora, F, bs, batch, incb):
    src = ora.uniform(batch * F * bs, 13, F + bs)
    dst = ora.uniform(F, 14, F + bs)
    ref = ora.add_sums(dst.copy(), src, batch, F, bs)
    scale = np.abs(src.reshape(batch, F, bs)).sum(axis=(0, 2)) + np.abs(dst)
    f64 = dst.astype(np.float64) + src.reshape(batch, F, bs).astype(np.float64).sum(axis=(0, 2))
    assert np.all(np.abs(ref - f64) <= 1e-5 * scale)
    full = np.full((F - 1) * incb + 1 + 4, SENT, np.float32)
    full[:(F - 1) * incb + 1:incb] = dst
    ddst = T.from_numpy(full.copy()).cuda()
    hip.backwardBias(F, ddst, src.size, T.from_numpy(src).cuda(), 0, incb, batch)
    hip.finish()
    got = ddst.cpu().numpy()
    assert np.array_equal(got[:(F - 1) * incb + 1:incb], ref)
    full[:(F - 1) * incb + 1:incb] = ref
    assert np.array_equal(got, full), "an element between the strided outputs changed"


@pytest.mark.parametrize("incb", [2, 3])
@pytest.mark.parametrize("F,bs,batch", [(3, 64, 5), (2, 333, 33), (2, 2047, 3), (2, 2048, 8),
                                         (3, 2053, 11), (2, 3080, 3), (2, 4099, 9), (1, 43264, 8),
                                         (5, 7, 3), (4, 1, 6), (1, 1, 333)])
def test_backward_bias_plain_kernel(hip, torch_cuda, ora, F, bs, batch, incb):
    """incb != 1 keeps backwardBias off the chain kernels: backward_bias_kernel
    at every block length (no full 8-block at bs = 7, long blocks, 33 groups =
    one past a 32-slot pass), writing dst[i * incb] and nothing between.
    (1, 1, 333): one output has no stride, so it stays the reference's
    stride-1 sumv (vssum_avx2 over the groups) whatever incb is; on this data
    the strided form's running sum rounds differently."""
    if F == 1 and bs == 1:
        src, run = ora.uniform(batch, 13, 2), np.float32(0)
        for v in src:
            run = np.float32(run + v)
        dst = ora.uniform(1, 14, 2)
        assert np.float32(dst[0] + run) != ora.add_sums(dst.copy(), src, batch, 1, 1)[0]
    _backward_bias_case(hip, torch_cuda, ora, F, bs, batch, incb)


@pytest.mark.parametrize("F,bs,batch", [(2, 9, 1025), (2, 63, 1100), (1, 8, 2049), (1, 1, 4099)])
def test_backward_bias_chunk_loop(hip, torch_cuda, ora, F, bs, batch):
    """incb = 1, bs < 64: backward_bias_kernel with more groups than one
    1024-group LDS chunk (last chunk of 1 group, of 76, three whole chunks);
    (1, 1, 4099) is the one-output FC sum, the same kernel over one long block."""
    _backward_bias_case(hip, torch_cuda, ora, F, bs, batch, 1)


@pytest.mark.parametrize("n", [N1, N4])
def test_activate_second_grid_trip(hip, torch_cuda, ora, big, n):
    x = big[0][:n]
    ref = ora.activate(x.copy(), 9)
    dx = torch_cuda.from_numpy(x.copy()).cuda()
    hip.ActivateArray(n, dx, 0, 9)
    hip.finish()
    assert same(dx.cpu().numpy(), ref)


@pytest.mark.parametrize("n", [N1, N4])
def test_derive_second_grid_trip(hip, torch_cuda, ora, big, n):
    y, delta = big[0][:n], big[1][:n]
    ref = ora.gradient(y.copy(), 9, delta.copy())
    dy, dd = torch_cuda.from_numpy(y.copy()).cuda(), torch_cuda.from_numpy(delta.copy()).cuda()
    hip.DeriveArray(n, dy, 0, 9, dd)
    hip.finish()
    assert same(dd.cpu().numpy(), ref)
    assert same(dy.cpu().numpy(), y), "DeriveArray wrote to x"


@pytest.mark.parametrize("F,bs,batch", [(7, 4 * 37, 16195), (7, 37, 16196)])  # float4, scalar
def test_forward_bias_second_grid_trip(hip, torch_cuda, ora, big, F, bs, batch):
    n = F * bs * batch
    assert n // (4 if bs % 4 == 0 else 1) > G and n <= N4
    x = big[0][:n]
    b = ora.uniform(F, 12, F, -0.1, 0.1)
    ref = ora.add_bias(x.copy(), b, F, bs, batch)
    dx = torch_cuda.from_numpy(x.copy()).cuda()
    hip.forwardBias(n, dx, 0, F, torch_cuda.from_numpy(b).cuda(), 1, batch)
    hip.finish()
    assert same(dx.cpu().numpy(), ref)


def test_blas1_second_grid_trip(hip, torch_cuda, ora, big):
    """axpy, scale, fill, copy, clamp, addvv, fmavv, fmavss, inverseSqrt past
    the 16384-block grid: whole arrays (axpy and scale are not idempotent, so
    an element visited twice shows as well as one that is skipped)."""
    T, n = torch_cuda, N1
    f32 = np.float32
    x, y = big[0][:n].copy(), big[1][:n].copy()
    dx, dy = T.from_numpy(x).cuda(), T.from_numpy(y.copy()).cuda()
    hip.axpy(n, 0.37, dx, 0, 1, dy, 0, 1)
    hip.finish()
    ref = y.copy()
    ora.lib().ora_saxpy(n, 0.37, x.ctypes.data, ref.ctypes.data)
    assert same(dy.cpu().numpy(), ref), "axpy"
    hip.scale(n, 2.5, dy, 1)
    hip.finish()
    ref = (ref * f32(2.5)).astype(f32)
    assert same(dy.cpu().numpy(), ref), "scale"
    dz = T.full((n + 3,), float(SENT), device="cuda")
    hip.copy(n, dy, 0, 1, dz, 0, 1)
    hip.finish()
    assert same(dz.cpu().numpy(), np.concatenate([ref, np.full(3, SENT, f32)])), "copy"
    hip.clamp(n, 1.25, dy, dz, 1, 0)
    hip.finish()
    assert same(dz.cpu().numpy()[:n], np.clip(ref, f32(-1.25), f32(1.25))), "clamp"
    hip.fill(n, dz, 0, 3.5, 1)
    hip.finish()
    assert same(dz.cpu().numpy(), np.concatenate([np.full(n, 3.5, f32), np.full(3, SENT, f32)])), \
        "fill"
    out = T.full((n,), float(SENT), device="cuda")
    hip.addvv(n, dx, 0, 1, dy, 0, 1, out, 0, 1)
    hip.finish()
    assert same(out.cpu().numpy(), x + ref), "addvv"
    hip.fmavv(n, dx, 0, 1, dy, 0, 1, dx, 0, 1, out, 0, 1)
    hip.finish()
    assert same(out.cpu().numpy(), ((x * ref).astype(f32) + x).astype(f32)), "fmavv"
    hip.fmavss(n, dx, 0, 1.5, -0.25, out)
    hip.finish()
    assert same(out.cpu().numpy(), ((x * f32(1.5)).astype(f32) + f32(-0.25)).astype(f32)), "fmavss"
    v = np.abs(x)
    v[::50] = 0.0
    hip.inverseSqrt(n, 0.0, T.from_numpy(v).cuda(), out, 1, 0)
    hip.finish()
    assert same(out.cpu().numpy(), (f32(1) / np.sqrt(np.maximum(v, f32(1e-6)))).astype(f32)), \
        "inverseSqrt"


@pytest.mark.parametrize("act", ALL_ACTS)
@pytest.mark.parametrize("off", [1, 2, 3])
def test_activate_misaligned(hip, torch_cuda, ora, act, off):
    """n % 4 == 0 at an element offset that is not: the scalar form, and
    nothing before or after the operand is touched."""
    n = 1024
    x = ora.uniform(n, 8, act, -6.0, 6.0)
    d = guarded(torch_cuda, x, off)
    hip.ActivateArray(n, d, off, act)
    hip.finish()
    assert same(unguard(d, off, n), ora.activate(x.copy(), act))


@pytest.mark.parametrize("act", ALL_ACTS)
@pytest.mark.parametrize("xoff,doff", [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (3, 1)])
def test_derive_misaligned(hip, torch_cuda, ora, act, xoff, doff):
    """launch_derive takes the float4 form only when both pointers are
    aligned: x misaligned through its offset with delta aligned, and the
    other way round."""
    n = 1024
    y = ora.activate(ora.uniform(n, 9, act, -3.0, 3.0), act)
    delta = ora.uniform(n, 10, act)
    dy, dd = guarded(torch_cuda, y, xoff), guarded(torch_cuda, delta, doff)
    hip.DeriveArray(n, dy, xoff, act, dd[doff:])
    hip.finish()
    assert same(unguard(dd, doff, n), ora.gradient(y, act, delta.copy()))
    assert same(unguard(dy, xoff, n), y)


def _derive_edges():
    f32 = np.float32
    y = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(f32(1), f32(0)),
                  np.nextafter(f32(-1), f32(0)), 0.5, -0.5], f32)
    y = np.concatenate([y, y])
    delta = np.array([1.5, -2.0, 0.75, -0.3, 3.0, -1.0, 2.0, 0.1] + [np.nan] * 8, f32)
    return y, delta


@pytest.mark.parametrize("n", [16, 15])  # float4 and scalar forms
@pytest.mark.parametrize("act", ALL_ACTS)
def test_derive_boundaries(hip, torch_cuda, ora, act, n):
    """gradient_array at the exact boundaries of every activation's pieces
    (y = +-0, +-1 and their float neighbours), and NaN deltas."""
    y, delta = (a[:n] for a in _derive_edges())
    ref = ora.gradient(y.copy(), act, delta.copy())
    dy, dd = torch_cuda.from_numpy(y.copy()).cuda(), torch_cuda.from_numpy(delta.copy()).cuda()
    hip.DeriveArray(n, dy, 0, act, dd)
    hip.finish()
    got = dd.cpu().numpy()
    assert same(got, ref), (act, got, ref)


@pytest.mark.parametrize("incb", [1, 2, 3])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_forward_bias_offsets_and_increments(hip, torch_cuda, ora, off, incb):
    """bs % 4 == 0 at every element offset (float4 form only at 0), bias read
    every incb elements."""
    F, bs, batch = 3, 8, 2
    x = ora.uniform(batch * F * bs, 11, off)
    b = ora.uniform((F - 1) * incb + 1, 12, incb, -0.1, 0.1)
    ref = ora.add_bias(x.copy(), b, F, bs, batch, incb)
    d = guarded(torch_cuda, x, off)
    hip.forwardBias(x.size, d, off, F, torch_cuda.from_numpy(b).cuda(), incb, batch)
    hip.finish()
    assert same(unguard(d, off, x.size), ref)


# bs >= 256 takes the *_rows kernels, smaller blocks scale_add_k / normalize_k
# (row_bpr, batchnorm.hip); bs % 4 == 0, so offset 0 is the float4 form
ROWS_AND_FLAT = [(2, 3, 260), (2, 3, 8)]


@pytest.mark.parametrize("incb", [1, 2, 3])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("groups,N,bs", ROWS_AND_FLAT)
def test_forward_scale_offsets_and_increments(hip, torch_cuda, ora, groups, N, bs, off, incb):
    T = torch_cuda
    x = ora.uniform(groups * N * bs, 21, off, -2.0, 3.0)
    s = ora.uniform((N - 1) * incb + 1, 22, incb, 0.5, 1.5)
    b = ora.uniform((N - 1) * incb + 1, 23, incb, -0.2, 0.2)
    sc = np.ascontiguousarray(s[::incb])
    y = ora.forward_scale(x.copy(), groups, N, bs, sc)
    d = guarded(T, x, off)
    hip.forwardScale(x.size, d, off, N, T.from_numpy(s).cuda(), incb, groups)
    hip.finish()
    assert same(unguard(d, off, x.size), y), "forwardScale"
    y2 = ora.add_bias(ora.forward_scale(y.copy(), groups, N, bs, sc), b, N, bs, groups, incb)
    hip.forwardScaleAdd(x.size, d, off, N, T.from_numpy(s).cuda(), T.from_numpy(b).cuda(), incb,
                        groups)
    hip.finish()
    assert same(unguard(d, off, x.size), y2), "forwardScaleAdd"


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("groups,N,bs", ROWS_AND_FLAT)
def test_normalize_offsets(hip, torch_cuda, ora, groups, N, bs, off, stride):
    T = torch_cuda
    x = ora.uniform(groups * N * bs, 24, off, -2.0, 3.0)
    m, v = ora.means_and_vars(x, groups, N, bs)
    ref = ora.normalize(x.copy(), groups, N, bs, m, v)
    ms, vs = np.full((N - 1) * stride + 1, SENT, np.float32), np.full(N * (stride + 1), SENT,
                                                                      np.float32)
    ms[::stride] = m
    vs[:N * (stride + 1):stride + 1] = v
    d = guarded(T, x, off)
    hip.normalize(N, x.size, groups, T.from_numpy(ms).cuda(), stride, T.from_numpy(vs).cuda(),
                  stride + 1, d, off)
    hip.finish()
    assert same(unguard(d, off, x.size), ref)


@pytest.mark.parametrize("act", [9, 4])
@pytest.mark.parametrize("offs", [(1, 0, 0), (0, 2, 0), (0, 0, 3), (3, 0, 0), (0, 1, 0), (0, 0, 2),
                                  (1, 2, 3)])
def test_shortcut_misaligned(hip, torch_cuda, ora, offs, act):
    """n % 4 == 0 with each operand misaligned on its own: the scalar form."""
    T, n = torch_cuda, 1024
    a, b = ora.uniform(n, 13, 0), ora.uniform(n, 13, 1)
    da, db = guarded(T, a, offs[0]), guarded(T, b, offs[1])
    do = guarded(T, np.full(n, SENT, np.float32), offs[2])
    hip.shortcut(n, da, offs[0], db, offs[1], do, offs[2], act)
    hip.finish()
    assert same(unguard(do, offs[2], n), ora.shortcut(a, b, act))
    assert same(unguard(da, offs[0], n), a) and same(unguard(db, offs[1], n), b)


@pytest.mark.parametrize("n", [N1, N4])
def test_shortcut_second_grid_trip(hip, torch_cuda, ora, big, n):
    T = torch_cuda
    a, b = big[0][:n], big[1][:n]
    out = T.full((n,), float(SENT), device="cuda")
    hip.shortcut(n, T.from_numpy(a.copy()).cuda(), 0, T.from_numpy(b.copy()).cuda(), 0, out, 0, 9)
    hip.finish()
    assert same(out.cpu().numpy(), ora.shortcut(a, b, 9))


def _strided(n, inc, off, seed, ora, tail=7):
    """A host buffer of random values with n live elements every inc from off."""
    buf = ora.uniform(off + (n - 1) * max(inc, 1) + 1 + tail, seed, n + inc)
    return buf


@pytest.mark.parametrize("n", [1, 255, 256, 257, 10007])
def test_blas1_offsets_and_strides(hip, torch_cuda, ora, n):
    """axpy / scale / fill / copy / clamp with increments 1, 2, 5 and
    non-zero offsets: the live elements bit-exact, every skipped element and
    everything around the operand unchanged."""
    T = torch_cuda
    f32 = np.float32
    live = lambda buf, off, inc: buf[off:off + (n - 1) * inc + 1:inc]  # noqa: E731
    for incx, incy, xo, yo in [(1, 1, 3, 5), (2, 1, 1, 2), (1, 2, 2, 1), (5, 2, 4, 3), (2, 5, 7, 9),
                               (0, 1, 6, 1), (0, 5, 2, 3)]:
        x, y = _strided(n, incx, xo, 15, ora), _strided(n, incy, yo, 16, ora)
        xs = live(x, xo, incx).copy() if incx else np.full(n, x[xo], f32)
        ys = live(y, yo, incy).copy()
        ora.lib().ora_saxpy(n, 0.37, xs.ctypes.data, ys.ctypes.data)
        ref = y.copy()
        live(ref, yo, incy)[:] = ys
        dx, dy = T.from_numpy(x).cuda(), T.from_numpy(y.copy()).cuda()
        hip.axpy(n, 0.37, dx, xo, incx, dy, yo, incy)
        hip.finish()
        assert same(dy.cpu().numpy(), ref), ("axpy", incx, incy)
        assert same(dx.cpu().numpy(), x), ("axpy wrote x", incx, incy)
    for inc, off in [(1, 3), (2, 1), (5, 6)]:
        x = _strided(n, inc, off, 17, ora)
        ref = x.copy()
        live(ref, off, inc)[:] = (live(x, off, inc) * f32(2.5)).astype(f32)
        dx = T.from_numpy(x.copy()).cuda()
        hip.scale(n, 2.5, dx[off:], inc)       # (scale takes no offset: a shifted pointer)
        hip.finish()
        assert same(dx.cpu().numpy(), ref), ("scale", inc)
        ref = x.copy()
        live(ref, off, inc)[:] = f32(-3.5)
        dx = T.from_numpy(x.copy()).cuda()
        hip.fill(n, dx, off, -3.5, inc)
        hip.finish()
        assert same(dx.cpu().numpy(), ref), ("fill", inc)
        # clamp: values at exactly +-alpha, just inside and outside, NaN, +-inf
        alpha = f32(0.625)
        edge = np.array([alpha, -alpha, np.nextafter(alpha, f32(1)), np.nextafter(-alpha, f32(-1)),
                         np.nextafter(alpha, f32(0)), np.nextafter(-alpha, f32(0)), np.nan, np.inf,
                         -np.inf, 0.0, -0.0], f32)
        x = _strided(n, inc, off, 18, ora)
        k = min(n, edge.size)
        live(x, off, inc)[:k] = edge[:k]
        cl = live(x, off, inc).copy()
        ora._lib2().ora_clamp(cl.ctypes.data, n, float(-alpha), float(alpha))
        ref = x.copy()
        live(ref, off, inc)[:] = cl
        dx = T.from_numpy(x.copy()).cuda()
        dst = T.full((x.size,), float(SENT), device="cuda")
        hip.clamp(n, float(alpha), dx, dst, inc, off)
        hip.finish()
        want = np.full(x.size, SENT, f32)
        live(want, off, inc)[:] = cl
        assert same(dst.cpu().numpy(), want), ("clamp", inc)
        hip.clamp(n, float(alpha), dx, dx, inc, off)   # in place
        hip.finish()
        assert same(dx.cpu().numpy(), ref), ("clamp in place", inc)
    for inca, incb, so, do in [(1, 1, 3, 5), (2, 1, 1, 2), (1, 5, 2, 1), (5, 2, 4, 3),
                               (0, 2, 3, 1)]:
        src, dst = _strided(n, inca, so, 19, ora), _strided(n, incb, do, 20, ora)
        ref = dst.copy()
        live(ref, do, incb)[:] = live(src, so, inca) if inca else src[so]
        ds, dd = T.from_numpy(src).cuda(), T.from_numpy(dst.copy()).cuda()
        hip.copy(n, ds, so, inca, dd, do, incb)
        hip.finish()
        assert same(dd.cpu().numpy(), ref), ("copy", inca, incb)


def test_elementwise_arg_errors_leave_the_operands_untouched(hip, torch_cuda):
    """Every argument guard of the BLAS-1 helpers, the bias / scale entry
    points and softmaxBatch raises TnsError ahead of any launch, as does an
    activation the library does not implement.  Each call points into the
    middle third of a sentinel buffer far larger than the operand, so the
    buffer shows a write even from a call that was let through."""
    from tensorium_amd._abi import TnsError
    T = torch_cuda
    third, n = 1024, 64
    a = T.full((3 * third,), float(SENT), device="cuda")
    b = T.full((3 * third,), float(SENT), device="cuda")
    m = third + third // 2                       # the middle of the buffer
    A, B = a[m:], b[m:]                          # shifted pointers, for the calls without offsets
    cases = {
        "axpy N<0": lambda: hip.axpy(-1, 2.0, a, m, 1, b, m, 1),
        "axpy null x": lambda: hip.axpy(n, 2.0, None, 0, 1, b, m, 1),
        "axpy null y": lambda: hip.axpy(n, 2.0, a, m, 1, None, 0, 1),
        "axpy incy 0": lambda: hip.axpy(n, 2.0, a, m, 1, b, m, 0),
        "axpy incy<0": lambda: hip.axpy(n, 2.0, a, m, 1, b, m, -2),
        "axpy incx<0": lambda: hip.axpy(n, 2.0, a, m, -1, b, m, 1),
        "scale N<0": lambda: hip.scale(-1, 2.0, A, 1),
        "scale null": lambda: hip.scale(n, 2.0, None, 1),
        "scale stride 0": lambda: hip.scale(n, 2.0, A, 0),
        "scale stride<0": lambda: hip.scale(n, 2.0, A, -3),
        "fill N<0": lambda: hip.fill(-1, a, m, 2.0, 1),
        "fill null": lambda: hip.fill(n, None, 0, 2.0, 1),
        "fill stride 0": lambda: hip.fill(n, a, m, 2.0, 0),
        "fill stride<0": lambda: hip.fill(n, a, m, 2.0, -1),
        "copy N<0": lambda: hip.copy(-1, a, m, 1, b, m, 1),
        "copy null src": lambda: hip.copy(n, None, 0, 1, b, m, 1),
        "copy null dst": lambda: hip.copy(n, a, m, 1, None, 0, 1),
        "copy incb 0": lambda: hip.copy(n, a, m, 1, b, m, 0),
        "copy incb<0": lambda: hip.copy(n, a, m, 1, b, m, -2),
        "copy inca<0": lambda: hip.copy(n, a, m, -1, b, m, 1),
        "clamp N<0": lambda: hip.clamp(-1, 1.0, a, b, 1, m),
        "clamp null src": lambda: hip.clamp(n, 1.0, None, b, 1, 0),
        "clamp null dst": lambda: hip.clamp(n, 1.0, a, None, 1, 0),
        "clamp stride 0": lambda: hip.clamp(n, 1.0, a, b, 0, m),
        "clamp stride<0": lambda: hip.clamp(n, 1.0, a, b, -2, m),
        "forwardBias incb 0": lambda: hip.forwardBias(n, a, m, 4, B, 0, 2),
        "forwardBias incb<0": lambda: hip.forwardBias(n, a, m, 4, B, -1, 2),
        "backwardBias incb 0": lambda: hip.backwardBias(4, A, n, b, m, 0, 2),
        "backwardBias incb<0": lambda: hip.backwardBias(4, A, n, b, m, -1, 2),
        "forwardScale incb 0": lambda: hip.forwardScale(n, a, m, 4, B, 0, 2),
        "forwardScale incb<0": lambda: hip.forwardScale(n, a, m, 4, B, -1, 2),
        "forwardScaleAdd incb 0": lambda: hip.forwardScaleAdd(n, a, m, 4, B, B[8:], 0, 2),
        "forwardScaleAdd incb<0": lambda: hip.forwardScaleAdd(n, a, m, 4, B, B[8:], -2, 2),
        "softmax stride 0": lambda: hip.softmaxBatch(8, a, m, 2, 16, 2, 8, 0, 1.0, b, m),
        "softmax stride<0": lambda: hip.softmaxBatch(8, a, m, 2, 16, 2, 8, -1, 1.0, b, m),
        "softmax batch<0": lambda: hip.softmaxBatch(8, a, m, -2, 16, 2, 8, 1, 1.0, b, m),
        "softmax groups<0": lambda: hip.softmaxBatch(8, a, m, 2, 16, -2, 8, 1, 1.0, b, m),
        "softmax batch_size<0": lambda: hip.softmaxBatch(8, a, m, 2, -16, 2, 8, 1, 1.0, b, m),
        "softmax group_size<0": lambda: hip.softmaxBatch(8, a, m, 2, 16, 2, -8, 1, 1.0, b, m),
        "softmax N<0": lambda: hip.softmaxBatch(-8, a, m, 2, 16, 2, 8, 1, 1.0, b, m),
        "activate act 2": lambda: hip.ActivateArray(n, a, m, 2),
        "derive act 2": lambda: hip.DeriveArray(n, a, m, 2, B),
        "shortcut act 2": lambda: hip.shortcut(n, a, m, b, m, b, m + 2 * n, 2),
    }
    passed = []
    for name, call in cases.items():
        try:
            call()
            passed.append(name)
        except TnsError:
            pass
    hip.finish()
    hip.lib.tns_clear_error()
    assert not passed, f"accepted: {passed}"
    sent = float(SENT)
    assert bool((a == sent).all()) and bool((b == sent).all()), "a refused call wrote to an operand"
    # what stays legal: empty calls, and a read increment of 0 (a broadcast)
    hip.axpy(0, 2.0, None, 0, 1, None, 0, 1)
    hip.scale(0, 2.0, None, 1)
    hip.fill(0, None, 0, 1.0, 1)
    hip.copy(0, None, 0, 1, None, 0, 1)
    hip.clamp(0, 1.0, None, None, 1, 0)
    hip.copy(n, a, m, 0, b, m, 1)
    hip.finish()
    assert bool((b == sent).all())
