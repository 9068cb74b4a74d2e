"""tns_conv_bf16_backward[_bn] and HipDarknetTrain(precision="bf16") against
float64 convolutions of the bf16-rounded operands.

A product of two bf16 values is exact in fp32, so the kernels' only error is
the fp32 accumulation of the n products and the prior value, in whatever
order: |got - ref| <= (n + 2) * 2^-23 * S + 2^-23, S the same sum over absolute
values (prior included), n = batch*oh*ow for dW and filters*k*k for dX.
"""
import numpy as np
import pytest

from _conv_bf16_ref import (BRANCH_CFG, BRANCH_CONVS, F, draw, held,
                            reference_backward as reference)
from tensorium_amd import darknet as dn
from tensorium_amd._abi import ACT

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 4

# C, H, W, filters, k, stride, pad, batch
CASES = [
    (8, 6, 6, 8, 3, 1, 0, 1),        # R = 16 < one reduction step, no padding, below one tile
    (3, 10, 7, 16, 3, 1, 1, 2),      # K = 27, H != W, an image boundary inside a step
    (32, 13, 13, 255, 1, 1, 0, 3),   # 1x1, filters one short; oh*ow = 169: pieces straddle images
    (40, 9, 11, 18, 3, 2, 1, 2),     # stride 2: dX's divisibility test, odd extents, K = 360
    (64, 26, 26, 130, 3, 1, 1, 1),   # several tiles both ways, 22 reduction steps: split 3 is real
    (96, 5, 5, 33, 1, 1, 0, 5),      # tiny planes, many images in a dX tile
]
# (dW split, dX tile): one varied while the other is by shape
FORMS = [(-1, -1), (1, -1), (3, -1), (-1, 0), (-1, 1)]
# ... and one case without state_delta
RUNS = [(c, s, t, True) for c in CASES for s, t in FORMS] + [(CASES[1], -1, -1, False)]


_DATA = {}


def case_data(torch, case):
    """The case's operands, prior buffers and reference, computed once."""
    if case not in _DATA:
        C, H, W, filters, k, stride, pad, batch = case
        oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        rng = np.random.default_rng(filters * 131 + C)
        x, w, d = draw(rng, batch, C, H, W), draw(rng, filters, C * k * k), \
            draw(rng, batch, filters, oh, ow)
        wu0, sd0, bu0 = draw(rng, filters, C * k * k), draw(rng, batch * C * H * W), \
            draw(rng, filters)
        _DATA[case] = (x, w, d, wu0, sd0, bu0, reference(torch, x, w, d, k, stride, pad, wu0, sd0))
    return _DATA[case]


@pytest.mark.parametrize("case,split,tile,with_sd", RUNS,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_backward(hip, torch_cuda, case, split, tile, with_sd):
    torch = torch_cuda
    C, H, W, filters, k, stride, pad, batch = case
    x, w, d, wu0, sd0, bu0, ((rw, bw), (rx, bx)) = case_data(torch, case)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dx_, dw_, out = dev(x), dev(w), torch.zeros(d.size, device="cuda")
    # LINEAR: delta passes the prologue unchanged; the fp32 call gives the bias sums
    bu_ref, ws = dev(bu0), torch.empty(batch * C * k * k * d[0, 0].size, device="cuda")
    hip.convBackward(batch, C, H, W, dx_, dw_, filters, k, stride, pad, 1, ACT["LINEAR"], out,
                     dev(d), bu_ref, dev(wu0), ws, None)
    hip.setConvBf16DwSplit(split)
    hip.setConvBf16Tile(tile)
    try:
        runs = []
        for _ in range(2):
            dd, bu, wu, sd = dev(d), dev(bu0), dev(wu0), dev(sd0)
            hip.convBackwardBf16(batch, C, H, W, dx_, dw_, filters, k, stride, pad, ACT["LINEAR"],
                                 out, dd, bu, wu, sd if with_sd else None)
            hip.finish()
            runs.append([t.cpu().numpy() for t in (wu, sd, bu, dd)])
    finally:
        hip.setConvBf16DwSplit(-1)
        hip.setConvBf16Tile(-1)
    what = f"{case} split {split} tile {tile}"
    held(runs[0][0], rw, bw, what + " dW")
    if with_sd:
        held(runs[0][1], rx, bx, what + " dX")
    else:
        assert np.array_equal(runs[0][1], sd0)
    assert np.array_equal(runs[0][2], bu_ref.cpu().numpy()) and np.array_equal(runs[0][3].ravel(),
                                                                               d.ravel())
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_backward_bn(hip, torch_cuda):
    torch = torch_cuda
    C, H, W, filters, k, stride, pad, batch = case = CASES[3]
    x, w, d, wu0, sd0, _, _ = case_data(torch, case)
    rng = np.random.default_rng(5)
    n = d.size
    host = dict(out=draw(rng, n), scales=draw(rng, filters), x=draw(rng, n), xn=draw(rng, n),
                mean=draw(rng, filters), var=np.abs(draw(rng, filters)) + F(0.5))
    dev = {k_: torch.from_numpy(v).cuda() for k_, v in host.items()}
    dx_, dw_ = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    res = []
    for bf16 in (False, True):
        dd, wu, sd = (torch.from_numpy(a).cuda() for a in (d, wu0, sd0))
        su, md, vd = (torch.zeros(filters, device="cuda") for _ in range(3))
        head = (batch, C, H, W, dx_, dw_, filters, k, stride, pad)
        tail = (ACT["LEAKY"], dev["out"], dd, dev["scales"], dev["x"], dev["xn"], dev["mean"],
                dev["var"], su, md, vd, wu)
        if bf16:
            hip.convBackwardBNBf16(*head, *tail, sd)
        else:
            hip.convBackwardBN(*head, 1, *tail, torch.empty(batch * C * k * k * n // filters,
                                                            device="cuda"), sd)
        hip.finish()
        res.append([t.cpu().numpy() for t in (dd, su, md, vd, wu, sd)])
    for a, b in zip(res[0][:4], res[1][:4]):  # the shared fp32 prologue
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    (rw, bw), (rx, bx) = reference(torch, x, w, res[1][0].reshape(d.shape), k, stride, pad, wu0,
                                   sd0)
    held(res[1][4], rw, bw, "bn dW")
    held(res[1][5], rx, bx, "bn dX")


@pytest.mark.parametrize("what", ["activation", "null weights", "overlap"])
def test_refusals(hip, torch_cuda, what):
    torch = torch_cuda
    C, H, filters = 8, 6, 8
    n = C * H * H
    buf = torch.full((4 * n + 2 * filters * C + filters,), 7.0, device="cuda")
    x, out, delta, sd, w, wu, bu = buf.split([n, n, n, n, filters * C, filters * C, filters])
    args = dict(act=ACT["LINEAR"], w=w.data_ptr(), sd=sd.data_ptr(), code=ERR_ARG)
    if what == "activation":
        args.update(act=ACT["ELU"], code=ERR_UNSUPPORTED)
    elif what == "null weights":
        args.update(w=None)
    else:
        args.update(sd=delta.data_ptr() + 4 * (n - 1))
    hip.lib.tns_clear_error()
    rc = hip.lib.tns_conv_bf16_backward(hip.ctx, 1, C, H, H, x.data_ptr(), args["w"], filters, 1,
                                        1, 0, args["act"], out.data_ptr(), delta.data_ptr(),
                                        bu.data_ptr(), wu.data_ptr(), args["sd"])
    assert rc == args["code"] and hip.lib.tns_last_error() != b""
    hip.lib.tns_clear_error()
    hip.finish()
    assert (buf.cpu().numpy() == 7.0).all()


def _conv(f, k, s, bn):
    return (f"[convolutional]\nbatch_normalize={bn}\nfilters={f}\nsize={k}\nstride={s}\npad=1\n"
            f"activation={'leaky' if bn else 'linear'}\n")


CFG = ("[net]\nbatch=2\nheight=32\nwidth=32\nchannels=3\n" + _conv(8, 3, 1, 1) + _conv(16, 3, 2, 1)
       + _conv(16, 1, 1, 0) + _conv(16, 3, 1, 0)
       + "[yolo]\nmask=0,1\nnum=2\nclasses=3\nanchors=4,4,8,8\n")


def test_train_driver(hip, torch_cuda):
    torch = torch_cuda
    net = dn.Network(dn.parse_cfg(CFG))
    params = dn.random_params(net, seed=11)
    with pytest.raises(ValueError):
        dn.HipDarknetTrain(hip, net, params, torch, precision="int8")
    tr = dn.HipDarknetTrain(hip, net, params, torch, precision="bf16")
    rng = np.random.default_rng(12)
    x = torch.from_numpy(draw(rng, 2, 3, 32, 32)).cuda()
    tr.forward(x)
    tr.set_yolo_deltas([torch.from_numpy(draw(rng, tr.delta[4].numel())).cuda()])
    host = lambda t: t.cpu().numpy().copy()  # noqa: E731
    before, after = {}, {}

    def snap(l):  # after layer l: what it left, and layer l-1's state_delta before it runs
        hip.finish()
        if l.kind == "convolutional":
            after[l.index] = (host(tr.delta[l.index]), host(tr.conv[l.index]["wu"]),
                              host(tr.delta[l.index - 1]) if l.index else None)
        if l.index >= 2:
            before[l.index - 1] = host(tr.delta[l.index - 2])
    tr.backward(x, on_backward=snap)
    convs = [l for l in net.layers if l.kind == "convolutional"]
    assert len(convs) == 4 and net.layers[-1].kind == "yolo"
    for l in convs:
        d, wu, sd = after[l.index]
        inp = host(x if l.index == 0 else tr.out[l.index - 1]).reshape(2, l.c, l.h, l.w)
        sd0 = before.get(l.index, np.zeros(inp.size, F))
        (rw, bw), (rx, bx) = reference(torch, inp, host(tr.conv[l.index]["w"]).reshape(l.filters, -1),
                                       d.reshape(2, l.filters, l.out_h, l.out_w), l.size,
                                       l.stride, l.pad, np.zeros(wu.shape), sd0)
        held(wu, rw.ravel(), bw.ravel(), f"layer {l.index} dW")
        if sd is not None:
            held(sd, rx, bx, f"layer {l.index} dX")


def test_train_driver_branches(hip, torch_cuda):
    """The backward through a net with branches: conv 2's output has three
    consumers (conv 3, the shortcut, the route), so conv 3's dX adds to a
    state_delta that is not zero; a maxpool and an upsample lie between convs.
    Every conv's dW and dX against the reference, the snapshot taken before
    the layer as dX's prior."""
    torch = torch_cuda
    net = dn.Network(dn.parse_cfg(BRANCH_CFG))
    params = dn.random_params(net, seed=21)
    tr = dn.HipDarknetTrain(hip, net, params, torch, precision="bf16")
    rng = np.random.default_rng(22)
    x = torch.from_numpy(draw(rng, 2, 3, 32, 32)).cuda()
    tr.forward(x)
    tr.set_yolo_deltas([torch.from_numpy(draw(rng, tr.delta[9].numel())).cuda()])
    host = lambda t: t.cpu().numpy().copy()  # noqa: E731
    before, after = {}, {}

    def snap(l):  # after layer l: what it left, and layer l-1's state_delta before it runs
        hip.finish()
        if l.kind == "convolutional":
            after[l.index] = (host(tr.delta[l.index]), host(tr.conv[l.index]["wu"]),
                              host(tr.delta[l.index - 1]) if l.index else None)
        if l.index >= 2:
            before[l.index - 1] = host(tr.delta[l.index - 2])
    tr.backward(x, on_backward=snap)
    convs = [l for l in net.layers if l.kind == "convolutional"]
    assert [l.index for l in convs] == BRANCH_CONVS
    # conv 3's input delta: the route's and the shortcut's terms are there before its dX
    assert np.count_nonzero(before[3]) > before[3].size // 2
    assert not before[8].any() and not before[2].any()
    for l in convs:
        d, wu, sd = after[l.index]
        inp = host(x if l.index == 0 else tr.out[l.index - 1]).reshape(2, l.c, l.h, l.w)
        sd0 = before.get(l.index, np.zeros(inp.size, F))
        (rw, bw), (rx, bx) = reference(torch, inp, host(tr.conv[l.index]["w"]).reshape(l.filters, -1),
                                       d.reshape(2, l.filters, l.out_h, l.out_w), l.size,
                                       l.stride, l.pad, np.zeros(wu.shape), sd0)
        print("group driver", held(wu, rw.ravel(), bw.ravel(), f"layer {l.index} dW"))
        if sd is not None:
            assert np.any(sd != sd0)
            print("group driver", held(sd, rx, bx, f"layer {l.index} dX"))
