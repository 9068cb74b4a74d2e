"""tns_conv_bf16_* and HipDarknet(precision="bf16") against a float64
convolution of the bf16-rounded operands.

A product of two bf16 values is exact in fp32, so the kernel's only error is
its fp32 accumulation (in whatever order) and the bias add: with S =
conv(|w~|, |x~|) + |b| and unit roundoff 2^-23 (which covers a truncating
accumulator), |y - ref| <= (K + 2) * 2^-23 * S + 2^-23 for the activations of
slope <= 1, the same with S / 4 for the logistic.
"""
import numpy as np
import pytest

from _conv_bf16_ref import BRANCH_CFG, BRANCH_CONVS, draw, held, reference_forward as reference
from tensorium_amd import darknet as dn
from tensorium_amd._abi import ACT

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 4

# C, H, W, filters, k, stride, pad, batch, activation
CASES = [
    (8, 6, 6, 8, 3, 1, 0, 1, "LINEAR"),       # below one tile, no padding, K = 72
    (3, 10, 7, 16, 3, 1, 1, 2, "LEAKY"),      # K = 27 < one k-step, H != W
    (32, 13, 13, 255, 1, 1, 0, 3, "LINEAR"),  # K one step, filters one short, images meet in a tile
    (40, 9, 11, 18, 3, 2, 1, 2, "LEAKY"),     # stride 2, K = 360 with a tail
    (64, 26, 26, 130, 3, 1, 1, 1, "RELU"),    # several tiles both ways, 18 k-steps
    (96, 5, 5, 33, 1, 1, 0, 5, "LOGISTIC"),   # tiny planes, many images in a tile, 3 k-steps
]
# the planner's pick, then each tile shape forced: every tile takes every case
TILES = [-1, 0, 1]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_forward(hip, torch_cuda, case, tile):
    torch = torch_cuda
    C, H, W, filters, k, stride, pad, batch, act = case
    act = ACT[act]
    rng = np.random.default_rng(filters * 131 + C)
    x, w, b = draw(rng, batch, C, H, W), draw(rng, filters, C * k * k), draw(rng, filters)
    ref, bound = reference(torch, x, w, b, k, stride, pad, act)
    dx, db = torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda()
    packed = hip.convBf16Pack(filters, C * k * k, torch.from_numpy(w).cuda())
    assert packed.numel() == hip.convBf16PackedBytes(filters, C * k * k)
    hip.setConvBf16Tile(tile)
    try:
        outs = []
        for _ in range(2):
            out = torch.full(ref.shape, np.nan, device="cuda")
            hip.convForwardBf16(batch, C, H, W, dx, packed, db, filters, k, stride, pad, act, out)
            hip.finish()
            outs.append(out.cpu().numpy())
    finally:
        hip.setConvBf16Tile(-1)
    held(outs[0], ref, bound, f"{case} tile {tile}")
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.parametrize("what", ["activation", "null packed", "overlap"])
def test_refusals(hip, torch_cuda, what):
    torch = torch_cuda
    C, H, filters = 8, 6, 8
    buf = torch.full((2 * C * H * H,), 7.0, device="cuda")
    x, out = buf[:C * H * H], buf[C * H * H:]
    packed = hip.convBf16Pack(filters, C, torch.zeros(filters * C, device="cuda"))
    bias = torch.zeros(filters, device="cuda")
    args = dict(act=ACT["LINEAR"], packed=packed.data_ptr(), out=out.data_ptr(), code=ERR_ARG)
    if what == "activation":
        args.update(act=ACT["ELU"], code=ERR_UNSUPPORTED)
    elif what == "null packed":
        args.update(packed=None)
    else:
        args.update(out=x.data_ptr() + 4 * (C * H * H - 1))
    hip.lib.tns_clear_error()
    rc = hip.lib.tns_conv_bf16_forward(hip.ctx, 1, C, H, H, x.data_ptr(), args["packed"],
                                       bias.data_ptr(), filters, 1, 1, 0, args["act"], args["out"])
    assert rc == args["code"] and hip.lib.tns_last_error() != b""
    hip.lib.tns_clear_error()
    hip.finish()
    assert (buf.cpu().numpy() == 7.0).all()


def _conv(f, k, s, bn):
    return (f"[convolutional]\nbatch_normalize={bn}\nfilters={f}\nsize={k}\nstride={s}\npad=1\n"
            f"activation={'leaky' if bn else 'linear'}\n")


CFG = ("[net]\nbatch=2\nheight=32\nwidth=32\nchannels=3\n" + _conv(8, 3, 1, 1)
       + "[maxpool]\nsize=2\nstride=2\n" + _conv(16, 3, 2, 1) + _conv(16, 1, 1, 0)
       + "[upsample]\nstride=2\n[route]\nlayers=-1,1\n" + _conv(16, 3, 1, 0)
       + "[yolo]\nmask=0,1\nnum=2\nclasses=3\nanchors=4,4,8,8\n")


def test_driver(hip, torch_cuda):
    torch = torch_cuda
    net = dn.Network(dn.parse_cfg(CFG))
    params = dn.random_params(net, seed=11)
    with pytest.raises(ValueError):
        dn.HipDarknet(hip, net, params, torch, precision="int8")
    x = torch.from_numpy(draw(np.random.default_rng(12), 2, 3, 32, 32)).cuda()
    out = dn.HipDarknet(hip, net, params, torch, precision="bf16").forward(x)
    hip.finish()
    convs = [l for l in net.layers if l.kind == "convolutional"]
    assert len(convs) == 4 and net.layers[-1].kind == "yolo"
    for l, p in zip(convs, params):
        f = dn.fuse_batchnorm(l, p)
        inp = (x if l.index == 0 else out[l.index - 1]).cpu().numpy().reshape(2, l.c, l.h, l.w)
        ref, bound = reference(torch, inp, f.weights.reshape(l.filters, -1), f.biases, l.size,
                               l.stride, l.pad, l.activation)
        held(out[l.index].cpu().numpy(), ref, bound, f"layer {l.index}")


def test_driver_branches(hip, torch_cuda):
    """A net with a shortcut, a route of two layers, a maxpool and an upsample
    between its convs, layer by layer."""
    torch = torch_cuda
    net = dn.Network(dn.parse_cfg(BRANCH_CFG))
    params = dn.random_params(net, seed=21)
    x = torch.from_numpy(draw(np.random.default_rng(22), 2, 3, 32, 32)).cuda()
    out = dn.HipDarknet(hip, net, params, torch, precision="bf16").forward(x)
    hip.finish()
    convs = [l for l in net.layers if l.kind == "convolutional"]
    assert [l.index for l in convs] == BRANCH_CONVS
    assert [net.layers[i].kind for i in (1, 4, 6, 7, 9)] == ["maxpool", "shortcut", "upsample",
                                                             "route", "yolo"]
    assert (convs[-1].c, convs[-1].h) == (32, 16)  # the route's two layers, upsampled
    for l, p in zip(convs, params):
        f = dn.fuse_batchnorm(l, p)
        inp = (x if l.index == 0 else out[l.index - 1]).cpu().numpy().reshape(2, l.c, l.h, l.w)
        ref, bound = reference(torch, inp, f.weights.reshape(l.filters, -1), f.biases, l.size,
                               l.stride, l.pad, l.activation)
        print("group driver", held(out[l.index].cpu().numpy(), ref, bound, f"layer {l.index}"))
