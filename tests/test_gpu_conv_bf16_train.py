"""tns_conv_bf16_forward_weights / _train: the bf16 MFMA product from the plain
fp32 weights against the float64 convolution of the bf16-rounded operands
(_conv_bf16_ref: |got - ref| <= (K + 2) * 2^-23 * S + 2^-23), against the
packed path bit for bit, and the batch-norm chain after it against the public
fp32 operations run on the stored product."""
import functools

import numpy as np
import pytest

from _conv_bf16_ref import TIE_CASES, held, operands, out_hw, reference_forward
from tensorium_amd._abi import ACT

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 4

# C, H, W, filters, k, stride, pad, batch; then the weights' offset in floats from a
# 16-byte boundary.  Beyond TIE_CASES, what the A loads can get wrong:
CASES = [(c, 0) for c in TIE_CASES] + [
    ((3, 5, 5, 1, 3, 1, 1, 1), 0),    # one filter; K = 27: 4-byte loads, one step partly past K
    ((4, 5, 4, 33, 3, 1, 0, 2), 0),   # 33 filters: a row into the second 32-row block; K = 36:
                                      # 16-byte loads, the second step holds 4 k
    ((8, 4, 4, 129, 3, 1, 1, 1), 0),  # 129 filters: one row in a second 128-row tile; K = 72
    ((8, 3, 3, 5, 3, 1, 0, 1), 0),    # batch * oh * ow = 1
    (TIE_CASES[0], 1),                # K = 72 a multiple of 4, the matrix off the boundary
]
IDS = ["x".join(map(str, c)) + f"+{o}" for c, o in CASES]


@functools.lru_cache(maxsize=None)
def _data(case):
    return operands(case, edges=True)


@functools.lru_cache(maxsize=None)
def _reference(torch, case, act):
    d, (_, _, _, _, k, stride, pad, _) = _data(case), case
    return reference_forward(torch, d["x"], d["w"], d["b"], k, stride, pad, act)


def _weights(torch, w, off):
    """w on the device, `off` floats behind a 16-byte boundary."""
    buf = torch.zeros(w.size + 4, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[off:off + w.size] = torch.from_numpy(w.reshape(-1)).cuda()
    return buf[off:off + w.size]


def _forward_weights(hip, torch, case, off, act, tile):
    C, H, W, filters, k, stride, pad, batch = case
    d = _data(case)
    oh, ow = out_hw(H, W, k, stride, pad)
    out = torch.full((batch, filters, oh, ow), np.nan, device="cuda")
    hip.setConvBf16Tile(tile)
    try:
        hip.convForwardBf16Weights(batch, C, H, W, torch.from_numpy(d["x"]).cuda(),
                                   _weights(torch, d["w"], off),
                                   torch.from_numpy(d["b"]).cuda(), filters, k, stride, pad, act,
                                   out)
        hip.finish()
    finally:
        hip.setConvBf16Tile(-1)
    return out


@pytest.mark.parametrize("act", ["LINEAR", "LEAKY", "LOGISTIC"])
@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("case,off", CASES, ids=IDS)
def test_forward_weights(hip, torch_cuda, case, off, tile, act):
    ref, bound = _reference(torch_cuda, case, ACT[act])
    out = _forward_weights(hip, torch_cuda, case, off, ACT[act], tile)
    held(out.cpu().numpy(), ref, bound, f"{case}+{off} tile {tile} {act}")


@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("case,off", CASES, ids=IDS)
def test_same_bits_as_packed(hip, torch_cuda, case, off, tile):
    """Both paths sum the same exact products in the same MFMA order."""
    torch = torch_cuda
    C, H, W, filters, k, stride, pad, batch = case
    d = _data(case)
    got = _forward_weights(hip, torch, case, off, ACT["LEAKY"], tile)
    packed = hip.convBf16Pack(filters, C * k * k, torch.from_numpy(d["w"]).cuda())
    want = torch.full_like(got, np.nan)
    hip.setConvBf16Tile(tile)
    try:
        hip.convForwardBf16(batch, C, H, W, torch.from_numpy(d["x"]).cuda(), packed,
                            torch.from_numpy(d["b"]).cuda(), filters, k, stride, pad, ACT["LEAKY"],
                            want)
        hip.finish()
    finally:
        hip.setConvBf16Tile(-1)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("case", [TIE_CASES[1], TIE_CASES[3]], ids=["3x3s1p1", "1x1f255"])
def test_forward_train(hip, torch_cuda, case):
    """x within the product's bound; every later buffer, and the inference
    call's out, bit for bit what the public fp32 operations give on that x."""
    torch = torch_cuda
    C, H, W, filters, k, stride, pad, batch = case
    d = _data(case)
    oh, ow = out_hw(H, W, k, stride, pad)
    n, mom, act = batch * filters * oh * ow, 0.1, ACT["LEAKY"]
    rng = np.random.default_rng(filters)
    up = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()  # noqa: E731
    sc, rm, rv = (up(rng.uniform(lo, hi, filters)) for lo, hi in ((.5, 1.5), (-.1, .1), (.5, 2)))
    dx, dw, bi = up(d["x"]), up(d["w"]), up(d["b"])

    def buffers(out):
        nan = lambda m: torch.full((m,), np.nan, device="cuda")  # noqa: E731
        return dict(mean=nan(filters), var=nan(filters), x=nan(n), xn=nan(n), rm=rm.clone(),
                    rv=rv.clone(), out=out)

    g = buffers(torch.full((n,), np.nan, device="cuda"))
    hip.convForwardTrainBf16(batch, C, H, W, dx, dw, filters, k, stride, pad, act, sc, bi,
                             g["rm"], g["rv"], mom, True, g["mean"], g["var"], g["x"], g["xn"],
                             g["out"])
    inference = torch.full((n,), np.nan, device="cuda")
    hip.convForwardTrainBf16(batch, C, H, W, dx, dw, filters, k, stride, pad, act, sc, bi, rm, rv,
                             mom, False, None, None, None, None, inference)
    hip.finish()
    ref, bound = reference_forward(torch, d["x"], d["w"], np.zeros_like(d["b"]), k, stride, pad,
                                   ACT["LINEAR"])
    held(g["x"].cpu().numpy(), ref, bound, f"{case} x")

    w = buffers(g["x"].clone())
    hip.meansAndVars(n, filters, batch, w["out"], 0, w["mean"], w["var"])
    for roll, stat in ((w["rm"], w["mean"]), (w["rv"], w["var"])):
        hip.scale(filters, float(np.float32(1) - np.float32(mom)), roll, 1)
        hip.axpy(filters, mom, stat, 0, 1, roll, 0, 1)
    hip.copy(n, w["out"], 0, 1, w["x"], 0, 1)
    hip.normalize(filters, n, batch, w["mean"], 1, w["var"], 1, w["out"], 0)
    hip.copy(n, w["out"], 0, 1, w["xn"], 0, 1)
    want_inference = g["x"].clone()
    hip.normalize(filters, n, batch, rm, 1, rv, 1, want_inference, 0)
    for out in (w["out"], want_inference):
        hip.forwardScaleAdd(n, out, 0, filters, sc, bi, 1, batch)
        hip.ActivateArray(n, out, 0, act)
    hip.finish()
    bits = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    for name in g:
        assert np.array_equal(bits(g[name]), bits(w[name])), name
    assert np.array_equal(bits(inference), bits(want_inference)), "inference"


# entry, what is wrong -> the code
REFUSALS = [(e, w) for e in ("weights", "train")
            for w in ("input", "weights", "biases", "out", "overlap", "size", "activation")]
REFUSALS += [("train", w) for w in ("scales", "rm", "x", "xn overlap")]


@pytest.mark.parametrize("entry,what", REFUSALS)
def test_refusals(hip, torch_cuda, entry, what):
    torch = torch_cuda
    C, H, filters = 8, 6, 8
    n = C * H * H
    buf = torch.full((5 * n + 6 * filters,), 7.0, device="cuda")
    p = {name: buf[i * n:].data_ptr() for i, name in enumerate(["input", "out", "x", "xn"])}
    p["weights"] = buf[4 * n:].data_ptr()  # filters * C <= n floats
    for i, name in enumerate(["biases", "scales", "rm", "rv", "mean", "var"]):
        p[name] = buf[5 * n + i * filters:].data_ptr()
    batch, act, code = 1, ACT["LINEAR"], ERR_ARG
    if what == "overlap":
        p["out"] = p["input"] + 4 * (n - 1)
    elif what == "xn overlap":
        p["xn"] = p["weights"] - 4 * (filters * H * H - 1)
    elif what == "size":
        batch = 0
    elif what == "activation":
        act, code = ACT["ELU"], ERR_UNSUPPORTED
    else:
        p[what] = None
    hip.lib.tns_clear_error()
    if entry == "weights":
        rc = hip.lib.tns_conv_bf16_forward_weights(hip.ctx, batch, C, H, H, p["input"],
                                                   p["weights"], p["biases"], filters, 1, 1, 0,
                                                   act, p["out"])
    else:
        rc = hip.lib.tns_conv_bf16_forward_train(hip.ctx, batch, C, H, H, p["input"], p["weights"],
                                                 filters, 1, 1, 0, act, p["scales"], p["biases"],
                                                 p["rm"], p["rv"], 0.1, 1, p["mean"], p["var"],
                                                 p["x"], p["xn"], p["out"])
    assert rc == code and hip.lib.tns_last_error() != b""
    hip.lib.tns_clear_error()
    hip.finish()
    assert (buf.cpu().numpy() == 7.0).all()
