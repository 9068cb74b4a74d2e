"""tns_image_bytes_to_input / tns_image_floats_to_input against the NumPy
restatement of TImageData.resize / letterBoxEx (tests/_image_oracle.py), bit
for bit.  dst stands between guard floats and the source rows between padding
that no pixel owns; both are checked after every call.  The size pairs reach:
the bottom-row quirk (2 -> 42 rows), w == 1, h == 1, an upscale, a downscale
over more than one block (53 columns at 64 a block row, 37 rows at 4), a mixed
up/down pair and the identity."""
import ctypes as C

import numpy as np
import pytest

from tensorium_amd._abi import TnsError

import _hazard_cases as hz
import _image_oracle as oracle

pytestmark = pytest.mark.gpu

F = np.float32
FILL = -7.0
GUARD = 64

# (source w, h) -> (target w, h)
PAIRS = [((5, 2), (7, 42)), ((1, 9), (6, 6)), ((9, 1), (6, 6)), ((2, 2), (13, 13)),
         ((53, 37), (32, 32)), ((37, 53), (53, 37)), ((37, 53), (37, 53))]
# (bytes?, channels, bytes a pixel)
KINDS = [(True, 1, 1), (True, 3, 3), (True, 3, 4), (True, 4, 4), (False, 1, 0), (False, 3, 0),
         (False, 4, 0)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(got, want, what):
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
    assert bad.size == 0, (what, bad[:8], np.asarray(got).reshape(-1)[bad[:8]],
                           np.asarray(want).reshape(-1)[bad[:8]])


def _pixels(rng, as_bytes, channels, ps, w, h):
    if as_bytes:
        return rng.integers(0, 256, (h, w, ps), dtype=np.uint8)
    return rng.random((channels, h, w), dtype=F)


def _pack(images, as_bytes, pad):
    """The images behind one another in one buffer, every row followed by
    `pad` elements no pixel owns (255 / NaN), GUARD more in front and behind.
    Returns (buffer, geom rows)."""
    parts, geom, at = [], [], GUARD
    junk = np.uint8(255) if as_bytes else F(np.nan)
    for im in images:
        if as_bytes:
            h, w, ps = im.shape
            rows = np.full((h, w * ps + pad), junk, np.uint8)
            rows[:, :w * ps] = im.reshape(h, w * ps)
        else:
            c, h, w = im.shape
            rows = np.full((c * h, w + pad), junk, F)
            rows[:, :w] = im.reshape(c * h, w)
        geom.append((at, w, h, rows.shape[1]))
        parts.append(rows.reshape(-1))
        at += rows.size
    g = np.full(GUARD, junk, dtype=parts[0].dtype)
    return np.concatenate([g, *parts, g]), geom


def _run(hip, torch, images, as_bytes, channels, ps, net, letter=False, table="fpc", pad=5):
    """One call; returns (dst [count, channels, netH, netW], placements) after
    checking the guards around dst and the whole source buffer."""
    buf, geom = _pack(images, as_bytes, pad)
    src = torch.from_numpy(buf).cuda()
    n = len(images) * channels * net[1] * net[0]
    whole = torch.full((n + 2 * GUARD,), FILL, device="cuda")
    placed = hip.imageToInput(src, geom, channels, net[0], net[1], whole[GUARD:GUARD + n],
                              letter=letter, table=table, pixelStride=ps if as_bytes else None)
    hip.finish()
    out = whole.cpu().numpy()
    assert (out[:GUARD] == F(FILL)).all() and (out[GUARD + n:] == F(FILL)).all(), "guards"
    assert np.array_equal(src.cpu().numpy().view(np.uint8), buf.view(np.uint8)), "source changed"
    return out[GUARD:GUARD + n].reshape(len(images), channels, net[1], net[0]), placed


def _planar(im, as_bytes, channels, table="fpc"):
    return oracle.planar_from_bytes(im, channels, table) if as_bytes else im


@pytest.mark.parametrize("src,dst", PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_resize_bit_exact(hip, torch_cuda, src, dst):
    rng = np.random.default_rng(11)
    for as_bytes, channels, ps in KINDS:
        im = _pixels(rng, as_bytes, channels, ps, *src)
        got, placed = _run(hip, torch_cuda, [im], as_bytes, channels, ps, dst)
        assert placed == [(dst[0], dst[1], 0, 0)]
        _same(got[0], oracle.resize(_planar(im, as_bytes, channels), *dst),
              (src, dst, as_bytes, channels, ps))


def test_bottom_row_quirk_reached(hip, torch_cuda):
    """5x2 -> 7x42: the device's last row is (1-dy)*P(0) with dy just below
    1, and not the source's last row."""
    im = np.full((1, 2, 5), F(0.75))
    got, _ = _run(hip, torch_cuda, [im], False, 1, 0, (7, 42))
    _, iy, dy = oracle.last_row(im, 42)
    assert iy == 0 and dy > F(0.999)
    _same(got[0], oracle.resize(im, 7, 42), "5x2 -> 7x42")
    assert got[0, :, -1, :].max() < 1e-5 and got[0, :, -2, :].min() > 0.7


@pytest.mark.parametrize("as_bytes,channels,ps", [(True, 3, 4), (False, 3, 0)])
def test_batch_of_three_sizes_in_one_call(hip, torch_cuda, as_bytes, channels, ps):
    rng = np.random.default_rng(12)
    sizes, net = [(5, 2), (53, 37), (2, 2)], (13, 19)
    ims = [_pixels(rng, as_bytes, channels, ps, w, h) for w, h in sizes]
    got, placed = _run(hip, torch_cuda, ims, as_bytes, channels, ps, net)
    assert placed == [(13, 19, 0, 0)] * 3
    for b, im in enumerate(ims):
        _same(got[b], oracle.resize(_planar(im, as_bytes, channels), *net), b)


def test_more_images_than_one_launch_takes(hip, torch_cuda):
    """kImagePerLaunch = 32 (csrc/tns_internal.hpp) images' geometry travel
    with one launch; 35 take two."""
    rng = np.random.default_rng(13)
    sizes = [(3 + b % 5, 2 + b % 7) for b in range(35)]
    ims = [_pixels(rng, True, 1, 1, w, h) for w, h in sizes]
    got, _ = _run(hip, torch_cuda, ims, True, 1, 1, (6, 5), pad=0)
    for b, im in enumerate(ims):
        _same(got[b], oracle.resize(_planar(im, True, 1), 6, 5), b)


@pytest.mark.parametrize("as_bytes,channels,ps", [(True, 3, 3), (False, 3, 0)])
def test_letterbox_bit_exact(hip, torch_cuda, as_bytes, channels, ps):
    rng = np.random.default_rng(14)
    sizes, net = [(50, 20), (20, 50), (30, 30)], (32, 32)
    ims = [_pixels(rng, as_bytes, channels, ps, w, h) for w, h in sizes]
    got, placed = _run(hip, torch_cuda, ims, as_bytes, channels, ps, net, letter=True)
    assert placed == [(32, 12, 0, 10), (12, 32, 10, 0), (32, 32, 0, 0)]
    for b, im in enumerate(ims):
        want, (nw, nh, dx, dy, _) = oracle.letterbox(_planar(im, as_bytes, channels), *net)
        assert placed[b] == (nw, nh, dx, dy)
        _same(got[b], want, b)
        border = np.ones((32, 32), bool)
        border[dy:dy + nh, dx:dx + nw] = False
        assert (got[b][:, border] == F(0.5)).all()
    assert (got[0][:, :10] == F(0.5)).all() and (got[1][:, :, 22:] == F(0.5)).all()


@pytest.mark.parametrize("table", ["fpc", "255", "own"])
def test_byte_tables(hip, torch_cuda, table):
    rng = np.random.default_rng(15)
    if table == "own":
        table = rng.standard_normal(256).astype(F)
    im = _pixels(rng, True, 3, 3, 53, 37)
    im[0, 0] = (0, 255, 128)
    got, _ = _run(hip, torch_cuda, [im], True, 3, 3, (32, 32), table=table)
    _same(got[0], oracle.resize(_planar(im, True, 3, table), 32, 32), "table")
    # (0, 0) is source pixel (0, 0) itself: the table's entries, untouched
    _same(got[0][:, 0, 0], oracle.byte_table(table)[[0, 255, 128]], "corner")


# ---- argument guards ---------------------------------------------------------
BASE = dict(count=1, off=0, w=8, h=8, rs=24, channels=3, ps=3, kind=0, table=False, net_w=6,
            net_h=6, letter=0, src=True, geom=True, dst=True)
BYTE_ERRORS = [
    dict(count=-1), dict(count=(1 << 20) + 1), dict(channels=0), dict(channels=5, ps=5, rs=40),
    dict(ps=2), dict(rs=23), dict(w=0), dict(h=0), dict(w=32769, rs=3 * 32769), dict(h=32769),
    dict(net_w=0), dict(net_h=0), dict(net_w=32769), dict(net_h=32769), dict(net_w=1),
    dict(net_h=1), dict(letter=1, w=1000, h=1, rs=3000), dict(letter=1, w=1, h=1000, rs=3),
    dict(off=-1), dict(kind=3), dict(kind=-1), dict(kind=2), dict(src=False), dict(geom=False),
    dict(dst=False)]
FLOAT_ERRORS = [
    dict(channels=0), dict(channels=1025), dict(rs=7), dict(w=0), dict(h=32769), dict(net_h=1),
    dict(letter=1, w=1000, h=1, rs=1000), dict(off=-1), dict(src=False), dict(geom=False),
    dict(dst=False)]


def _raw(hip, torch, as_bytes, over):
    a = dict(BASE, rs=24 if as_bytes else 8)
    a.update(over)
    src = torch.zeros(4096, dtype=torch.uint8 if as_bytes else torch.float32, device="cuda")
    dst = torch.full((4096,), FILL, device="cuda")
    geom = (C.c_int64 * 4)(a["off"], a["w"], a["h"], a["rs"])
    placed = (C.c_int64 * 4)(-9, -9, -9, -9)
    ptr = lambda t, on: t.data_ptr() if on else None                     # noqa: E731
    if as_bytes:
        rc = hip.lib.tns_image_bytes_to_input(
            hip.ctx, a["count"], ptr(src, a["src"]), geom if a["geom"] else None, a["channels"],
            a["ps"], a["kind"], None, a["net_w"], a["net_h"], a["letter"], ptr(dst, a["dst"]),
            placed)
    else:
        rc = hip.lib.tns_image_floats_to_input(
            hip.ctx, a["count"], ptr(src, a["src"]), geom if a["geom"] else None, a["channels"],
            a["net_w"], a["net_h"], a["letter"], ptr(dst, a["dst"]), placed)
    hip.lib.tns_clear_error()
    hip.finish()
    return rc, dst, list(placed)


_ids = lambda o: "-".join(f"{k}={v}" for k, v in o.items())                # noqa: E731


@pytest.mark.parametrize("over", BYTE_ERRORS, ids=_ids)
def test_byte_argument_guards(hip, torch_cuda, over):
    rc, dst, placed = _raw(hip, torch_cuda, True, over)
    assert rc == 1                                                       # TNS_ERR_ARG
    assert (dst == FILL).all().item() and placed == [-9] * 4


@pytest.mark.parametrize("over", FLOAT_ERRORS, ids=_ids)
def test_float_argument_guards(hip, torch_cuda, over):
    rc, dst, placed = _raw(hip, torch_cuda, False, over)
    assert rc == 1
    assert (dst == FILL).all().item() and placed == [-9] * 4


def test_the_guards_base_call_is_good(hip, torch_cuda):
    """What every guard case departs from succeeds, and so does count == 0
    with nothing else given."""
    for as_bytes in (True, False):
        rc, dst, placed = _raw(hip, torch_cuda, as_bytes, {})
        assert rc == 0 and placed == [6, 6, 0, 0]
        assert (dst[:3 * 36] == 0).all().item() and (dst[3 * 36:] == FILL).all().item()
        rc, dst, placed = _raw(hip, torch_cuda, as_bytes,
                               dict(count=0, src=False, geom=False, dst=False))
        assert rc == 0 and placed == [-9] * 4


def test_wrapper_refuses_a_bad_table(hip, torch_cuda):
    src = torch_cuda.zeros(64, dtype=torch_cuda.uint8, device="cuda")
    dst = torch_cuda.zeros(3 * 36, device="cuda")
    for bad in ("256", [0.0] * 255):
        with pytest.raises(TnsError, match="table"):
            hip.imageToInput(src, [(0, 4, 4, 12)], 3, 6, 6, dst, table=bad)


# ---- the side stream ---------------------------------------------------------
@pytest.mark.parametrize("as_bytes", [True, False], ids=["bytes", "floats"])
def test_a_call_joins_the_pending_dw(hip, torch_cuda, as_bytes):
    """The pending state as tests/test_gpu_hazards.py builds it: a pipelined
    conv backward (TNS_OPT_BWD_OVERLAP = 2, im2col + sdot dW) leaves its dW on
    the side stream.  The image entries touch nothing of it and join all the
    same: they are outside the hazard table and take its conservative side."""
    T = torch_cuda
    i = np.arange(hz.ARENA, dtype=np.int64)
    arena = T.from_numpy((0.25 + 0.5 * ((i * 37) % 101) / 101.0).astype(F)).cuda()
    v = lambda at, n: arena[at:at + n]                                   # noqa: E731
    at = {r.name: r.r0 for r in hz.PENDING}
    src = T.zeros(256, dtype=T.uint8 if as_bytes else T.float32, device="cuda")
    dst = T.empty(3 * 36, device="cuda")
    try:
        hip.setBwdOverlap(2)
        hip.setDwRes(-2)
        hip.setDwTile(-2)
        hip.finish()
        hip.convBackward(hz.PB, hz.PC, hz.PH, hz.PH, v(at["input"], hz.P_IN),
                         v(hz.HOME_WEIGHTS, hz.P_W), hz.PF, hz.PK, 1, 1, 1, hz.LEAKY,
                         v(hz.HOME_OUTPUT, hz.P_OUT), v(at["delta"], hz.P_OUT),
                         v(hz.HOME_BIAS_UPDATES, hz.PF), v(at["weight_updates"], hz.P_W),
                         v(at["col"], hz.P_COL), None)
        assert hip.pendingDw() == 1, "precondition: the conv backward left its dW pending"
        hip.imageToInput(src, [(0, 4, 4, 12 if as_bytes else 4)], 3, 6, 6, dst)
        assert hip.pendingDw() == 0
    finally:
        hip.finish()
        hip.setDwRes(-1)
        hip.setDwTile(-1)
        hip.setBwdOverlap(True)
        hip.finish()
