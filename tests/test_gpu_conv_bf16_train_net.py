"""HipDarknetTrain(forward_precision="bf16") on the net with branches: the first
convolution's product against the float64 reference, one whole training step,
and the default spelled out against the default left out."""
import numpy as np
import pytest

from _conv_bf16_ref import BRANCH_CFG, draw, held, reference_forward
from tensorium_amd import darknet as dn
from tensorium_amd._abi import ACT

pytestmark = pytest.mark.gpu


def _step(hip, torch, **kw):
    net = dn.Network(dn.parse_cfg(BRANCH_CFG))
    tr = dn.HipDarknetTrain(hip, net, dn.random_params(net, seed=21), torch, **kw)
    rng = np.random.default_rng(22)
    x = torch.from_numpy(draw(rng, 2, 3, 32, 32)).cuda()
    tr.forward(x)
    hip.finish()
    x0 = tr.conv[0]["x"].cpu().numpy()  # the net input's product, before any update
    tr.set_yolo_deltas([torch.from_numpy(draw(rng, tr.delta[9].numel())).cuda()])
    tr.backward(x)
    tr.update(1e-3, 0.9, 5e-4)
    hip.finish()
    return net, tr, x, x0


def test_first_product_and_one_step(hip, torch_cuda):
    torch = torch_cuda
    net, tr, x, x0 = _step(hip, torch, forward_precision="bf16")
    l, w = net.layers[0], dn.random_params(net, seed=21)[0].weights
    ref, bound = reference_forward(torch, x.cpu().numpy(), w.reshape(l.filters, -1),
                                   np.zeros(l.filters, np.float32), l.size, l.stride, l.pad,
                                   ACT["LINEAR"])
    held(x0, ref, bound, "conv 0 x")
    for st in tr.conv.values():
        for name in ("w", "b", "scales", "rm", "rv"):
            assert name not in st or np.isfinite(st[name].cpu().numpy()).all(), name


def test_fp32_is_the_default(hip, torch_cuda):
    (_, a, _, ax), (_, b, _, bx) = (_step(hip, torch_cuda, **kw)
                                    for kw in ({}, {"forward_precision": "fp32"}))
    assert np.array_equal(ax.view(np.uint32), bx.view(np.uint32))
    for i, st in a.conv.items():
        for name, t in st.items():
            assert np.array_equal(t.cpu().numpy().view(np.uint32),
                                  b.conv[i][name].cpu().numpy().view(np.uint32)), (i, name)
    for i in range(len(a.out)):
        assert np.array_equal(a.out[i].cpu().numpy(), b.out[i].cpu().numpy()), i
