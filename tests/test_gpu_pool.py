"""Max and local-average pooling on the HIP backend against the CPU checker
(tests/_pool_oracle.py), bit for bit, stored indexes included.

Geometries: the smallest that reach every path of csrc/pool.hip — windows
that leave the input on each side, overlapping windows (the backward's add
order), two different strides, the 2x2/2 form (W a multiple of 8) with an even
and an odd H, float4 and scalar stores, more than one block with a tail, and
buffers that are not 16-byte aligned.  Backward deltas are u*10^e, e in
[-3, 3], on a non-zero state.delta: for the overlapping geometries the test
first shows, on the checker alone, that the descending order gives other bits,
so a wrong order cannot pass."""
import numpy as np
import pytest

from tensorium_amd._abi import TnsError

import _pool_oracle as po

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(np.finfo(np.float32).max)

# name: (B, C, H, W), size, stride_x, stride_y, padding
GEOMS = {
    "2x2s2_odd": ((2, 3, 7, 9), 2, 2, 2, 0),        # unused last row and column
    "2x2s1_pad1": ((2, 3, 5, 7), 2, 1, 1, 1),       # last windows partly outside
    "3x3s2_pad2": ((2, 3, 9, 10), 3, 2, 2, 2),      # off = -1: top and left outside
    "5x5s1_pad4": ((2, 3, 6, 6), 5, 1, 1, 4),       # heavy overlap (SPP)
    "3x3_sx1_sy2": ((2, 3, 9, 11), 3, 1, 2, 2),
    "blocks_tail": ((2, 5, 33, 37), 2, 2, 2, 1),    # W % 4 != 0, > 1 block, a tail
    "blocks_overlap": ((2, 5, 33, 37), 3, 1, 1, 2),
    "fast_2x2": ((2, 3, 8, 16), 2, 2, 2, 1),        # W % 8 == 0: the 2x2/2 form
    "fast_2x2_oddh": ((2, 3, 7, 16), 2, 2, 2, 1),   # its second row outside at the end
    "fast_2x2_blocks": ((2, 8, 32, 32), 2, 2, 2, 0),
    "vec_general": ((2, 3, 6, 8), 2, 1, 1, 1),      # general form, float4 stores
}
OVERLAP = [k for k, (_, size, sx, sy, _) in GEOMS.items() if sx < size or sy < size]


def _input(name, kind):
    shape = GEOMS[name][0]
    rng = np.random.default_rng(sorted(GEOMS).index(name) * 10 + len(kind))
    if kind == "ties":      # 4 levels: most windows hold their maximum more than once
        return (rng.integers(0, 4, shape) / 4).astype(np.float32)
    x = rng.uniform(-1, 1, shape).astype(np.float32)
    if kind == "specials":
        f = x.reshape(-1)
        for v in (np.nan, np.inf, -np.inf, -FLT_MAX):
            f[rng.choice(f.size, max(4, f.size // 12), replace=False)] = v
        # one window holding only NaN: output 0's (and whatever shares its taps)
        _, size, sx, sy, pad = GEOMS[name]
        x[0, 0, :max(1, size - pad // 2), :max(1, size - pad // 2)] = np.nan
    return x


def _deltas(rng, shape):
    return (rng.uniform(-1, 1, shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32)


def _dev(torch, a, misalign=False):
    """A device copy; misalign: at an address that is 4 (float32) or 8 (int64)
    bytes past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(-1)
    if not misalign:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    buf[1:].copy_(t)
    v = buf[1:]
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def _geom_args(name):
    (B, C, H, W), size, sx, sy, pad = GEOMS[name]
    oh, ow = po.out_shape(H, W, size, sx, sy, pad)
    return B, C, H, W, size, sx, sy, pad, oh, ow


def _run_max(hip, torch, name, x, sd0, d, misalign=False, with_idx=True):
    B, C, H, W, size, sx, sy, pad, oh, ow = _geom_args(name)
    X = _dev(torch, x, misalign)
    out = _dev(torch, np.full(B * C * oh * ow, 7, np.float32), misalign)
    idx = _dev(torch, np.full(B * C * oh * ow, -7, np.int64), misalign) if with_idx else None
    hip.forwardMaxPool(B, C, oh, ow, X, C, H, W, sx, sy, pad, size, idx, out)
    if not with_idx:
        return out.cpu().numpy(), None, None
    SD, D = _dev(torch, sd0, misalign), _dev(torch, d, misalign)
    hip.backwardMaxPool(B, C, oh, ow, SD, idx, D, H, W, sx, sy, pad, size)
    return out.cpu().numpy(), idx.cpu().numpy(), SD.cpu().numpy()


def _check_max(hip, torch, name, kind, misalign=False):
    (shape, size, sx, sy, pad) = GEOMS[name]
    x = _input(name, kind)
    rng = np.random.default_rng(99)
    ref_out, ref_idx = po.maxpool_forward(x, size, sx, sy, pad)
    d = _deltas(rng, ref_out.shape)
    sd0 = rng.uniform(-1, 1, shape).astype(np.float32)
    ref_sd = sd0.copy()
    po.maxpool_backward(ref_sd, ref_idx, d)
    if name in OVERLAP and kind != "specials":
        wrong = sd0.copy()
        po.maxpool_backward(wrong, ref_idx, d, descending=True)
        assert not np.array_equal(wrong, ref_sd), "the case does not tell the add order"
    if kind == "specials":
        assert ref_idx.ravel()[0] == -1 and ref_out.ravel()[0] == -FLT_MAX
        assert np.isinf(ref_out).any()
    out, idx, sd = _run_max(hip, torch, name, x, sd0, d, misalign)
    assert np.array_equal(out, ref_out.ravel())
    assert np.array_equal(idx, ref_idx.ravel())
    assert np.array_equal(sd, ref_sd.ravel())
    # inference: null indexes, the same output
    out2, _, _ = _run_max(hip, torch, name, x, sd0, d, misalign, with_idx=False)
    assert np.array_equal(out2, ref_out.ravel())


@pytest.mark.parametrize("kind", ["random", "ties", "specials"])
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_maxpool_forward_backward(hip, torch_cuda, name, kind):
    _check_max(hip, torch_cuda, name, kind)


@pytest.mark.parametrize("name", ["fast_2x2", "vec_general", "blocks_overlap"])
def test_maxpool_unaligned_buffers(hip, torch_cuda, name):
    """Every buffer 4 (8: indexes) bytes past a 16-byte boundary: the scalar
    forms, the same bits."""
    _check_max(hip, torch_cuda, name, "ties", misalign=True)


def _check_avg(hip, torch, name, misalign=False):
    B, C, H, W, size, sx, sy, pad, oh, ow = _geom_args(name)
    x = _input(name, "random")
    rng = np.random.default_rng(98)
    ref_out = po.avgpool_forward(x, size, sx, sy, pad)
    d = _deltas(rng, ref_out.shape)
    sd0 = rng.uniform(-1, 1, x.shape).astype(np.float32)
    ref_sd = sd0.copy()
    po.avgpool_backward(ref_sd, d, x.shape, size, sx, sy, pad)
    if name in OVERLAP:
        wrong = sd0.copy()
        po.avgpool_backward(wrong, d, x.shape, size, sx, sy, pad, descending=True)
        assert not np.array_equal(wrong, ref_sd), "the case does not tell the add order"
    X, SD, D = _dev(torch, x, misalign), _dev(torch, sd0, misalign), _dev(torch, d, misalign)
    out = _dev(torch, np.full(ref_out.size, 7, np.float32), misalign)
    hip.forwardAvgPool(B, C, oh, ow, X, C, H, W, sx, sy, pad, size, out)
    hip.backwardAvgPool(B, C, oh, ow, SD, D, H, W, sx, sy, pad, size)
    assert np.array_equal(out.cpu().numpy(), ref_out.ravel())
    assert np.array_equal(SD.cpu().numpy(), ref_sd.ravel())


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_avgpool_forward_backward(hip, torch_cuda, name):
    _check_avg(hip, torch_cuda, name)


def test_avgpool_unaligned_buffers(hip, torch_cuda):
    _check_avg(hip, torch_cuda, "fast_2x2", misalign=True)
    _check_avg(hip, torch_cuda, "vec_general", misalign=True)


@pytest.mark.parametrize("name", ["2x2s2_odd", "fast_2x2"])   # scalar and float4 rows
def test_backward_writes_only_named_elements(hip, torch_cuda, name):
    """An element no stored index names keeps its bits — a NaN payload that
    an add would not return unchanged."""
    torch = torch_cuda
    B, C, H, W, size, sx, sy, pad, oh, ow = _geom_args(name)
    x = _input(name, "random")
    _, ref_idx = po.maxpool_forward(x, size, sx, sy, pad)
    sd0 = np.full(x.size, 0x7fa00001, np.uint32).view(np.float32)   # a signalling NaN
    named = np.zeros(x.size, bool)
    named[ref_idx.ravel()] = True
    sd0 = np.where(named, np.float32(1), sd0).astype(np.float32)
    assert np.array_equal(sd0.view(np.uint32)[~named], np.full((~named).sum(), 0x7fa00001))
    d = np.ones(ref_idx.size, np.float32)
    SD, D, I = _dev(torch, sd0), _dev(torch, d), _dev(torch, ref_idx)
    hip.backwardMaxPool(B, C, oh, ow, SD, I, D, H, W, sx, sy, pad, size)
    got = SD.cpu().numpy()
    assert np.array_equal(got[named], np.full(named.sum(), 2, np.float32))
    assert np.array_equal(got.view(np.uint32)[~named], sd0.view(np.uint32)[~named])


# (entry, what is wrong): geometry overrides on a valid 2x3x6x8 size 2 stride 2
# padding 0 call
BAD = [
    dict(size=0), dict(size=-1), dict(sx=0), dict(sy=0), dict(pad=-1), dict(B=-1), dict(H=-1),
    dict(c=4),                      # outC != c
    dict(oh=4), dict(ow=3),         # not the shape the geometry gives
    dict(size=9, oh=1, ow=1),       # beyond the padded input
    dict(H=65536, W=65536, oh=32768, ow=32768),   # a plane beyond 2^31 elements
    dict(null="out"), dict(null="in"),
]


def _bad_call(kw):
    g = dict(B=2, C=3, H=6, W=8, size=2, sx=2, sy=2, pad=0, oh=3, ow=4, c=3, null=None)
    g.update(kw)
    return g


@pytest.mark.parametrize("kw", BAD, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_bad_geometry_rejected_before_any_write(hip, torch_cuda, kw):
    torch = torch_cuda
    g = _bad_call(kw)
    x = torch.ones(2 * 3 * 6 * 8, device="cuda")
    out = torch.full((2 * 3 * 3 * 4,), 7.0, device="cuda")
    idx = torch.full((2 * 3 * 3 * 4,), -7, dtype=torch.int64, device="cuda")
    sd = torch.full((2 * 3 * 6 * 8,), 5.0, device="cuda")
    d = torch.ones(2 * 3 * 3 * 4, device="cuda")
    xin = None if g["null"] == "in" else x
    o = None if g["null"] == "out" else out
    with pytest.raises(TnsError, match="tns status 1"):
        hip.forwardMaxPool(g["B"], g["C"], g["oh"], g["ow"], xin, g["c"], g["H"], g["W"], g["sx"],
                           g["sy"], g["pad"], g["size"], idx, o)
    with pytest.raises(TnsError, match="tns status 1"):
        hip.forwardAvgPool(g["B"], g["C"], g["oh"], g["ow"], xin, g["c"], g["H"], g["W"], g["sx"],
                           g["sy"], g["pad"], g["size"], o)
    if "c" not in kw:   # (the backward has no c to disagree with)
        dd = None if g["null"] == "in" else d
        s = None if g["null"] == "out" else sd
        with pytest.raises(TnsError, match="tns status 1"):
            hip.backwardMaxPool(g["B"], g["C"], g["oh"], g["ow"], s, idx, dd, g["H"], g["W"],
                                g["sx"], g["sy"], g["pad"], g["size"])
        with pytest.raises(TnsError, match="tns status 1"):
            hip.backwardAvgPool(g["B"], g["C"], g["oh"], g["ow"], s, dd, g["H"], g["W"], g["sx"],
                                g["sy"], g["pad"], g["size"])
    assert bool((out == 7).all()) and bool((idx == -7).all()) and bool((sd == 5).all())


def test_more_rejections(hip, torch_cuda):
    torch = torch_cuda
    out = torch.full((16,), 7.0, device="cuda")
    x = torch.ones(16, device="cuda")
    # avg: size 1, padding 2 on 4x4 -> off = -1, window (0, 0) lies outside the input
    with pytest.raises(TnsError, match="no tap inside"):
        hip.forwardAvgPool(1, 1, 6, 6, x, 1, 4, 4, 1, 1, 2, 1, torch.full((36,), 7.0,
                                                                          device="cuda"))
    with pytest.raises(TnsError, match="no tap inside"):
        hip.backwardAvgPool(1, 1, 6, 6, out, torch.ones(36, device="cuda"), 4, 4, 1, 1, 2, 1)
    # ... which the max pool takes: -FLT_MAX and -1 there
    o = torch.full((36,), 7.0, device="cuda")
    i = torch.full((36,), -7, dtype=torch.int64, device="cuda")
    hip.forwardMaxPool(1, 1, 6, 6, x, 1, 4, 4, 1, 1, 2, 1, i, o)
    ro, ri = po.maxpool_forward(np.ones((1, 1, 4, 4), np.float32), 1, 1, 1, 2)
    assert np.array_equal(o.cpu().numpy(), ro.ravel()) and np.array_equal(i.cpu().numpy(),
                                                                          ri.ravel())
    assert ri.ravel()[0] == -1 and ri.ravel()[7] == 0
    # maxpool backward without indexes; operands of the wrong type
    with pytest.raises(TnsError, match="null operand"):
        hip.backwardMaxPool(1, 1, 2, 2, out, None, x, 4, 4, 2, 2, 0, 2)
    with pytest.raises(TnsError, match="int64"):
        hip.forwardMaxPool(1, 1, 2, 2, x, 1, 4, 4, 2, 2, 0, 2, torch.zeros(4, device="cuda"), out)
    with pytest.raises(TnsError, match="float32"):
        hip.forwardMaxPool(1, 1, 2, 2, x, 1, 4, 4, 2, 2, 0, 2, None,
                           torch.zeros(4, dtype=torch.int64, device="cuda"))
    assert bool((out == 7).all())
    # nothing to do is not an error
    hip.forwardMaxPool(0, 1, 2, 2, None, 1, 4, 4, 2, 2, 0, 2, None, None)
    hip.backwardMaxPool(0, 1, 2, 2, None, None, None, 4, 4, 2, 2, 0, 2)
