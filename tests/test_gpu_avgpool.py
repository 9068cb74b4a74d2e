"""The global average pool kernels (csrc/pool.hip) against the CPU checker
(tests/_avgpool_oracle.py), bit for bit through a uint32 view.

Shapes (planes, n): the smallest that reach every path — n below one block of
eight (tail only), whole blocks only, blocks plus a tail, the four-blocks-ahead
loop with a remainder (49, 169, 1031), fewer planes than the eight of a wave
and than the 32 of a block, and two with more planes than one trip of the
grid covers (forward: 2048 blocks of 32 planes; backward: 2048 blocks of 256
float4 groups).  Every shape is run with the input and state.delta at element
offsets 0, 1 and 3 of a larger buffer (the backward's scalar head and tail at
every alignment) and with planted planes: all -0.0, one NaN, one +Inf, and a
cancellation pattern whose result depends on the order."""
import numpy as np
import pytest

from tensorium_amd._abi import TnsError

import _avgpool_oracle as ao

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = [(1, 1), (3, 7), (8, 8), (9, 9), (5, 15), (13, 49), (64, 64), (24, 169), (5, 1031),
          (70001, 9), (70001, 31)]
KINDS = ("negzero", "nan", "inf", "cancel")
GUARD = f32(7.25)
CANCEL = np.array([1e8, 1, -1e8, 0.5, 1, 0.25, 3, -2], f32)   # repeated along the plane


def plant(x, kind, p):
    n = x.shape[1]
    if kind == "negzero":
        x[p] = -0.0
    elif kind == "nan":
        x[p, n // 2] = np.nan
    elif kind == "inf":
        x[p, n - 1] = np.inf
    else:
        x[p] = np.resize(CANCEL, n)


def plans(planes):
    """Which plane holds which planted case: all four at once where there
    are planes enough, else one run per case."""
    if planes >= 5:   # spread over the first wave's planes and the last plane
        return [dict(zip(KINDS, (1, 2, 3, planes - 1)))]
    return [{k: planes - 1} for k in KINDS]


_cache = {}


def case(ora, planes, n, which):
    """Input, forward reference, delta, state.delta before and after: computed
    once per (shape, plan), read only."""
    key = (planes, n, which)
    if key not in _cache:
        rng = np.random.default_rng(1000 * n + planes + which)
        x = rng.standard_normal((planes, n)).astype(f32)
        for kind, p in plans(planes)[which].items():
            plant(x, kind, p)
        out = ao.forward(ora, x, planes, n)
        d = (rng.standard_normal(planes) * 10.0 ** rng.integers(-3, 4, planes)).astype(f32)
        sd0 = rng.standard_normal(planes * n).astype(f32)
        sd0[rng.random(planes * n) < 0.2] = -0.0
        for kind, p in plans(planes)[which].items():   # the same cases as deltas
            if kind != "cancel":
                d[p] = {"negzero": -0.0, "nan": np.nan, "inf": np.inf}[kind]
        sd = sd0.copy()
        ao.backward(sd, d, planes, n)
        for a in (x, out, d, sd0, sd):
            a.setflags(write=False)
        _cache[key] = (x, out, d, sd0, sd)
    return _cache[key]


def based(torch, a, off, tail=5):
    """a at element offset off of a buffer of guards; (buffer, view)."""
    buf = torch.full((off + a.size + tail,), float(GUARD), device="cuda")
    view = buf[off:off + a.size]
    view.copy_(torch.from_numpy(np.array(a, f32, copy=True).reshape(-1)))
    return buf, view


def guards_ok(buf, off, size):
    g = buf.cpu().numpy()
    return bool((g[:off] == GUARD).all() and (g[off + size:] == GUARD).all())


def bits(a):
    return np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("planes,n", SHAPES)
def test_forward_backward(hip, torch_cuda, ora, planes, n, off):
    torch = torch_cuda
    for which in range(len(plans(planes))):
        x, ref_out, d, sd0, ref_sd = case(ora, planes, n, which)
        if "negzero" in plans(planes)[which]:
            p = plans(planes)[which]["negzero"]
            assert ref_out[p] == 0 and not np.signbit(ref_out[p])
        _, X = based(torch, x, off)
        obuf, O = based(torch, np.full(planes, 3, f32), 4 - off)
        hip.forwardGlobalAvgPool(planes, 1, n, 1, X, O)
        assert np.array_equal(bits(O.cpu().numpy()), bits(ref_out)), (which, "forward")
        assert guards_ok(obuf, 4 - off, planes)
        assert np.array_equal(bits(X.cpu().numpy()), bits(x))
        sbuf, SD = based(torch, sd0, off)
        _, D = based(torch, d, (off + 2) % 4)
        hip.backwardGlobalAvgPool(1, planes, 1, n, D, SD)
        assert np.array_equal(bits(SD.cpu().numpy()), bits(ref_sd)), (which, "backward")
        assert guards_ok(sbuf, off, planes * n)
        assert np.array_equal(bits(D.cpu().numpy()), bits(d))


def test_the_cancellation_plane_depends_on_the_order(ora):
    for n in sorted({n for _, n in SHAPES if n >= 3}):
        x = np.resize(CANCEL, n).astype(f32)[None]
        got = ao.forward(ora, x, 1, n)[0]
        assert got != f32(np.mean(x.astype(np.float64))), n


def _operands(torch):
    x = torch.arange(24, dtype=torch.float32, device="cuda")
    small = torch.full((6,), 5.0, device="cuda")
    return x, small


BAD = [
    dict(B=-1), dict(c=-2, B=3), dict(h=-4), dict(h=(1 << 24) + 1, w=1, B=1, c=1),
    dict(B=1 << 20, c=1 << 20, h=1 << 12, w=1 << 12),   # planes*n*8 beyond 2^63
    dict(null="big"), dict(null="small"),
    dict(overlap=0), dict(overlap=23), dict(overlap=-5),   # first, last and first element shared
]


@pytest.mark.parametrize("kw", BAD, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_bad_arguments_rejected_before_any_write(hip, torch_cuda, kw):
    torch = torch_cuda
    g = dict(B=2, c=3, h=2, w=2, null=None, overlap=None)
    g.update(kw)
    for forward in (True, False):
        big, small = _operands(torch)
        b = None if g["null"] == "big" else big
        s = None if g["null"] == "small" else small
        if g["overlap"] is not None:   # six floats from this element of the big operand
            s = big.data_ptr() + 4 * g["overlap"]
        with pytest.raises(TnsError, match="tns status 1"):
            if forward:
                hip.forwardGlobalAvgPool(g["B"], g["c"], g["h"], g["w"], b, s)
            else:
                hip.backwardGlobalAvgPool(g["B"], g["c"], g["h"], g["w"], s, b)
        hip.finish()
        assert np.array_equal(big.cpu().numpy(), np.arange(24, dtype=f32))
        assert bool((small == 5).all())


def test_touching_operands_are_accepted(hip, torch_cuda, ora):
    """The small operand right before and right after the big one."""
    torch = torch_cuda
    x = np.arange(24, dtype=f32)
    ref = ao.forward(ora, x, 6, 4)
    for lo in (True, False):
        buf = torch.zeros(30, device="cuda")
        big = buf[6:] if lo else buf[:24]
        small = buf[:6] if lo else buf[24:]
        big.copy_(torch.from_numpy(x))
        hip.forwardGlobalAvgPool(2, 3, 2, 2, big, small)
        assert np.array_equal(small.cpu().numpy(), ref)


def test_zero_sizes_do_nothing(hip, torch_cuda):
    torch = torch_cuda
    big, small = _operands(torch)
    for B, c, h, w in ((0, 3, 2, 2), (2, 0, 2, 2), (2, 3, 0, 2), (2, 3, 2, 0), (0, 0, 0, 0)):
        hip.forwardGlobalAvgPool(B, c, h, w, big, small)
        hip.backwardGlobalAvgPool(B, c, h, w, small, big)
        hip.forwardGlobalAvgPool(B, c, h, w, None, None)
        hip.backwardGlobalAvgPool(B, c, h, w, None, None)
    hip.finish()
    assert np.array_equal(big.cpu().numpy(), np.arange(24, dtype=f32))
    assert bool((small == 5).all())
