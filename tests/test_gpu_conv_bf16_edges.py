"""The bf16 convolution kernels (conv_bf16.hip, conv_bf16_bwd.hip) on the
shapes, activations and values their first tests leave out, against the same
float64 references and derived bounds (tests/_conv_bf16_ref.py).

What each case reaches is worked out from the planners as they stand: by shape
conv_bf16_pick gives the 64 x 64 tile to every case here (none has 512 large
tiles), conv_bf16_dw_split gives one slice (fewer than 16 reduction steps; the
13 x 13 tie case has 16 and gets two), and conv_bf16_dw_tile gives the 64 x 64
tile unless a case says otherwise; the other tile and the other splits are
forced.  tests/test_conv_bf16_ref.py checks these statements without a GPU.
"""
import numpy as np
import pytest

from _conv_bf16_ref import (F, TIE_CASES, draw, held, operands, out_hw, reference_backward,
                            reference_forward)
from tensorium_amd._abi import ACT

pytestmark = pytest.mark.gpu

TILES = [-1, 0, 1]
# (dW split, dX tile): one varied while the other is by shape
FORMS = [(-1, -1), (1, -1), (3, -1), (-1, 0), (-1, 1)]

# C, H, W, filters, k, stride, pad, batch
GEOMETRY = [
    # dX's divide path (sshift < 0) at stride 3: ty, tx negative and not multiples of 3; 4 x 3
    # outputs whose windows leave a row and a column of the padded 13 x 10 image unused; dX has
    # 3 k-steps (Kd = 90) and 3 column tiles of 64 (2 of 128); dW one step (R = 24)
    (12, 11, 8, 10, 3, 3, 1, 2),
    # ... and at stride 4 under a 5 x 5 kernel with pad 2 (windows overlap by one): taps up to
    # ty = -4; Kd = 175: 6 k-steps with a tail of 15; dW one step (R = 18), K = 150: 3 tiles
    (6, 9, 9, 7, 5, 4, 2, 2),
    # dX over C = 136: two channel tiles under 128 x 128 (rows 128..135 of the second), three
    # under 64 x 64 (the last 8 rows of 64), W^T packed to 256 rows; N = 150: two / three column
    # tiles, so blockIdx.x % mtiles and / mtiles both vary; dW: K = 1224, 20 column tiles of 64
    (136, 6, 5, 9, 3, 1, 1, 5),
    # oh = ow = 1: every reduction element of dW is another image (R = 11: one piece and a
    # half, the rest of the step invalid); the forward's and dX's column decode at ohw = 1
    (4, 3, 3, 5, 3, 1, 0, 11),
    # 1 x 3 planes: a dW piece crosses two image ends (R = 9)
    (4, 3, 5, 5, 3, 1, 0, 3),
    # oh = ow = 1 at stride 2 and R = 1: one valid element in the whole reduction
    (5, 4, 4, 6, 3, 2, 0, 1),
    # an even kernel (k = 2, stride 2, pad 0): kk = 4 in the pack kernels' (f, ky, kx) walk
    (6, 8, 10, 9, 2, 2, 0, 2),
    # k = 5, pad 2: taps ky, kx up to 4 in the k-tables, 25 taps a filter in the W^T pack
    (5, 9, 7, 12, 5, 1, 2, 2),
    # k = 7, stride 2, pad 3 on 3 channels (a first layer): K = 147, Kd = 980 (31 k-steps)
    (3, 17, 15, 20, 7, 2, 3, 1),
    # 1 x 1 with pad 1: an output border that is bias alone; dX taps off both sides
    (10, 5, 6, 8, 1, 1, 1, 2),
    # 3 x 3 with pad 2: corner windows wholly in the padding
    (7, 4, 5, 6, 3, 1, 2, 2),
]
# dW's 128 x 128 tile (filters = 130 >= 128, K = 144 >= 128: 2 x 2 tiles) across images: oh*ow =
# 49, R = 147 = 5 steps, every step and most pieces straddle an image end.  Split 1: the kernel
# adds into weight_updates; 2: slices of 3 and 2 steps; 5: the step count, one step a slice
DW128 = (16, 7, 7, 130, 3, 1, 1, 3)
DW128_SPLITS = [1, 2, 5]
# the activations' shape: stride 2, K = 360 with a tail, odd extents
ACT_CASE = (40, 9, 11, 18, 3, 2, 1, 2)

ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731
WORST = {}


def record(group, worst):
    """The groups' worst max err / bound, printed for DESIGN.md's record."""
    WORST[group] = max(WORST.get(group, 0.0), worst)
    print("group", group, "worst max err / bound so far", WORST[group])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32).ravel(),
                          np.ascontiguousarray(b, F).view(np.uint32).ravel())


_FWD, _BWD = {}, {}


def forward_data(torch, case, act, edges=False, wscale=1.0):
    """The case's operands and forward reference, computed once."""
    key = (case, act, edges, wscale)
    if key not in _FWD:
        C, H, W, filters, k, stride, pad, batch = case
        o = operands(case, edges)
        w = (o["w"] * F(wscale)).astype(F)
        _FWD[key] = (o["x"], w, o["b"],
                     reference_forward(torch, o["x"], w, o["b"], k, stride, pad, ACT[act]))
    return _FWD[key]


def run_forward(hip, torch, case, act, tile, data, group):
    C, H, W, filters, k, stride, pad, batch = case
    x, w, b, (ref, bound) = data
    dx, dw, db = (torch.from_numpy(a).cuda() for a in (x, w, b))
    packed = hip.convBf16Pack(filters, C * k * k, dw)
    hip.setConvBf16Tile(tile)
    try:
        outs = []
        for _ in range(2):
            out = torch.full(ref.shape, np.nan, device="cuda")
            hip.convForwardBf16(batch, C, H, W, dx, packed, db, filters, k, stride, pad, ACT[act],
                                out)
            hip.finish()
            outs.append(out.cpu().numpy())
    finally:
        hip.setConvBf16Tile(-1)
    record(group, held(outs[0], ref, bound, f"{case} {act} tile {tile}"))
    assert same_bits(outs[0], outs[1])
    assert same_bits(dx.cpu().numpy(), x) and same_bits(dw.cpu().numpy(), w)


def backward_data(torch, case, edges=False):
    """The case's operands, prior buffers and LINEAR backward reference, once."""
    key = (case, edges)
    if key not in _BWD:
        k, stride, pad = case[4:7]
        o = operands(case, edges)
        _BWD[key] = (o, reference_backward(torch, o["x"], o["w"], o["d"], k, stride, pad, o["wu0"],
                                           o["sd0"]))
    return _BWD[key]


def run_backward(hip, torch, case, split, tile, o, group, act="LINEAR", refs=None):
    """Two bf16 calls and one fp32 call on the same inputs.  delta after the
    call and bias_updates must have the fp32 entry's bits (the shared fp32
    prologue), dW and dX must hold their bounds against the reference of the
    prepared delta, input / weights / output must be untouched and the two
    calls must agree bit for bit.  Returns the first call's (wu, sd)."""
    C, H, W, filters, k, stride, pad, batch = case
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out_h = o["out"] if "out" in o else np.zeros(o["d"].size, F)
    dx_, dw_, out = dev(o["x"]), dev(o["w"]), dev(out_h)
    d32, bu32 = dev(o["d"]), dev(o["bu0"])
    hip.convBackward(batch, C, H, W, dx_, dw_, filters, k, stride, pad, 1, ACT[act], out, d32,
                     bu32, dev(o["wu0"]), None, None)
    hip.finish()
    d_ref, bu_ref = d32.cpu().numpy(), bu32.cpu().numpy()
    hip.setConvBf16DwSplit(split)
    hip.setConvBf16Tile(tile)
    try:
        runs = []
        for _ in range(2):
            dd, bu, wu, sd = dev(o["d"]), dev(o["bu0"]), dev(o["wu0"]), dev(o["sd0"])
            hip.convBackwardBf16(batch, C, H, W, dx_, dw_, filters, k, stride, pad, ACT[act], out,
                                 dd, bu, wu, sd)
            hip.finish()
            runs.append([t.cpu().numpy() for t in (wu, sd, bu, dd)])
    finally:
        hip.setConvBf16DwSplit(-1)
        hip.setConvBf16Tile(-1)
    what = f"{case} {act} split {split} tile {tile}"
    assert same_bits(runs[0][2], bu_ref), what + " bias_updates"
    assert same_bits(runs[0][3], d_ref), what + " delta"
    if act == "LINEAR":
        assert same_bits(d_ref, o["d"])
    else:
        refs = reference_backward(torch, o["x"], o["w"], d_ref.reshape(o["d"].shape), k, stride,
                                  pad, o["wu0"], o["sd0"])
    (rw, bw), (rx, bx) = refs
    record(group, held(runs[0][0], rw, bw, what + " dW"))
    record(group, held(runs[0][1], rx, bx, what + " dX"))
    for a, b in zip(*runs):
        assert same_bits(a, b), what
    for t, h in ((dx_, o["x"]), (dw_, o["w"]), (out, out_h)):
        assert same_bits(t.cpu().numpy(), h), what + ": an input was written"
    return runs[0][:2]


# ---- geometry (the issue's gaps 1 - 5) ---------------------------------------------
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", GEOMETRY + [DW128], ids=ids)
def test_forward_geometry(hip, torch_cuda, case, tile):
    run_forward(hip, torch_cuda, case, "LEAKY", tile, forward_data(torch_cuda, case, "LEAKY"),
                "geometry")


@pytest.mark.parametrize("split,tile", FORMS, ids=ids)
@pytest.mark.parametrize("case", GEOMETRY, ids=ids)
def test_backward_geometry(hip, torch_cuda, case, split, tile):
    o, refs = backward_data(torch_cuda, case)
    run_backward(hip, torch_cuda, case, split, tile, o, "geometry", refs=refs)


@pytest.mark.parametrize("split", DW128_SPLITS)
def test_backward_dw128(hip, torch_cuda, split):
    o, refs = backward_data(torch_cuda, DW128)
    run_backward(hip, torch_cuda, DW128, split, -1, o, "geometry", refs=refs)


# ---- activations (gap 6) --------------------------------------------------------------
# the weights scaled by 1/16: pre-activations of deviation ~0.4, so tanh and the logistic are off
# their flat ends and hardtan clamps a few outputs at either end, not most
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("act", ["TANH", "REVLEAKY", "HARDTAN"])
def test_forward_activations(hip, torch_cuda, act, tile):
    data = forward_data(torch_cuda, ACT_CASE, act, wscale=1 / 16)
    if act == "HARDTAN":
        assert (data[3][0] == 1.0).any() and (data[3][0] == -1.0).any()
        assert (np.abs(data[3][0]) < 1.0).any()
    run_forward(hip, torch_cuda, ACT_CASE, act, tile, data, "activations")


@pytest.mark.parametrize("split,tile", FORMS, ids=ids)
@pytest.mark.parametrize("act", ["LEAKY", "LOGISTIC", "TANH"])
def test_backward_activations(hip, torch_cuda, act, split, tile):
    o = dict(operands(ACT_CASE))
    # the layer's output as the activation leaves it: in (0, 1) for the logistic, (-1, 1) else
    v = draw(np.random.default_rng(6), o["d"].size)
    o["out"] = ((v + 1) / 2).astype(F) if act == "LOGISTIC" else v
    run_backward(hip, torch_cuda, ACT_CASE, split, tile, o, "activations", act=act)


# ---- operand rounding (gap 7) ------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", TIE_CASES, ids=ids)
def test_forward_ties(hip, torch_cuda, case, tile):
    run_forward(hip, torch_cuda, case, "LINEAR", tile,
                forward_data(torch_cuda, case, "LINEAR", edges=True), "tie data")


@pytest.mark.parametrize("split,tile", FORMS, ids=ids)
@pytest.mark.parametrize("case", TIE_CASES, ids=ids)
def test_backward_ties(hip, torch_cuda, case, split, tile):
    o, refs = backward_data(torch_cuda, case, edges=True)
    run_backward(hip, torch_cuda, case, split, tile, o, "tie data", refs=refs)


# ---- the context's scratch and k-table cache across calls (gap 8) -------------------------
def test_backward_scratch_sequence(hip, torch_cuda):
    """One context, in sequence: DW128 in three slices (the dW partials and the
    W^T scratch at their largest), a tiny case with neither split nor much
    W^T, DW128 again (the same bits as the first time), then a case with C ==
    filters and oh == H, ow == W: its two k-tables are one cache entry."""
    tiny, shared = GEOMETRY[3], (8, 6, 6, 8, 3, 1, 1, 2)
    assert shared[0] == shared[3] and out_hw(*shared[1:3], *shared[4:7]) == shared[1:3]
    got = []
    for case, split in ((DW128, 3), (tiny, -1), (DW128, 3), (shared, -1)):
        o, refs = backward_data(torch_cuda, case)
        got.append(run_backward(hip, torch_cuda, case, split, -1, o, "scratch sequence", refs=refs))
    for a, b in zip(got[0], got[2]):
        assert same_bits(a, b)
