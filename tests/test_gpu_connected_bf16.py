"""The connected layer's three products on the bf16 GEMM (connected.py with a
bf16 state) and the drivers' connected_precision="bf16", against the float64
products of the bf16-rounded operands and the bound of tests/_gemm_bf16_ref.py.
"""
import numpy as np
import pytest

from _conv_bf16_ref import F, draw, held
from _gemm_bf16_ref import reference
from tensorium_amd import darknet as dn
from tensorium_amd._abi import ACT
from tensorium_amd.darknet import connected as fc

pytestmark = pytest.mark.gpu
S, T, I, O = 3, 2, 20, 33  # rows a step, steps, inputs, outputs


def _state(hip, torch, rng, training):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, F)).cuda()  # noqa: E731
    z = lambda n: torch.zeros(n, device="cuda")  # noqa: E731
    p = dn.ConvParams(np.zeros(O, F), draw(rng, O, I))  # zero bias: the product alone
    return p, t, fc.state(t, z, p, O, I, ACT["LINEAR"], False, T * S, training, hip=hip,
                          precision="bf16")


@pytest.mark.parametrize("training", [False, True])
def test_forward_at_step_1(hip, torch_cuda, training):
    """Non-zero offsets into inp and out; the inference state holds packed weights."""
    rng = np.random.default_rng(5 + training)
    p, t, st = _state(hip, torch_cuda, rng, training)
    assert st.bf16 and ("wp" in st) == (not training) and ("w" in st) == training
    inp = draw(rng, T * S, I)
    fc.forward(hip, st, S, 1, t(inp.ravel()), 1, training)
    hip.finish()
    out = st["out"].cpu().numpy().reshape(T * S, O)
    ref, bound = reference("NT", inp[S:], p.weights, np.zeros((S, O)))
    held(out[S:], ref, bound, "forward")
    assert not out[:S].any()


def test_backward_at_step_1(hip, torch_cuda):
    rng = np.random.default_rng(7)
    p, t, st = _state(hip, torch_cuda, rng, True)
    inp, d, wu0, sd0 = draw(rng, T * S, I), draw(rng, T * S, O), draw(rng, O, I), draw(rng, T * S, I)
    st["delta"].copy_(t(d.ravel()))
    st["wu"].copy_(t(wu0.ravel()))
    sd = t(sd0.ravel())
    fc.backward(hip, st, S, 1, t(inp.ravel()), 1, sd, 1)  # LINEAR, |delta| <= 1: delta as drawn
    hip.finish()
    held(st["wu"].cpu().numpy(), *reference("TN", d[S:], inp[S:], wu0), "weight_updates")
    sd = sd.cpu().numpy().reshape(T * S, I)
    held(sd[S:], *reference("NN", d[S:], p.weights, sd0[S:]), "state.delta")
    assert np.array_equal(sd[:S], sd0[:S])


CFG = ("[net]\nbatch=3\ninputs=20\n[connected]\noutput=33\nactivation=leaky\n"
       "[connected]\noutput=7\nactivation=linear\n[softmax]\n")


def test_driver(hip, torch_cuda):
    torch = torch_cuda
    net = dn.Network(dn.parse_cfg(CFG))
    params = dn.random_params(net, seed=11)
    for cls in (dn.HipDarknet, dn.HipDarknetTrain):
        with pytest.raises(ValueError):
            cls(hip, net, params, torch, connected_precision="int8")
    rng = np.random.default_rng(12)
    x = torch.from_numpy(draw(rng, 3, 20)).cuda()
    host = lambda v: v.cpu().numpy().copy()  # noqa: E731
    layers = net.layers[:2]

    def check_forward(out, what):  # each layer from its actual input; leaky's slope is <= 1
        for l, p in zip(layers, params):
            inp = host(x if l.index == 0 else out[l.index - 1]).reshape(3, l.in_size)
            y, bound = reference("NT", inp, p.weights.reshape(l.filters, -1),
                                 np.tile(p.biases.astype(np.float64), (3, 1)))
            ref = np.where(y < 0, 0.1 * y, y) if l.activation == ACT["LEAKY"] else y
            held(host(out[l.index]), ref, bound, f"{what} layer {l.index}")

    model = dn.HipDarknet(hip, net, params, torch, connected_precision="bf16")
    assert all("wp" in st and "w" not in st for st in model.fc.values())
    out = model.forward(x)
    hip.finish()
    check_forward(out, "inference")

    tr = dn.HipDarknetTrain(hip, net, params, torch, connected_precision="bf16")
    truth = np.zeros((3, 7), F)
    truth[np.arange(3), [1, 4, 6]] = 1
    tr.forward(x, torch.from_numpy(truth).cuda())
    hip.finish()
    check_forward(tr.out, "training")
    after = {}

    def snap(l):  # after layer l: its delta as the products read it, wu, the delta below
        hip.finish()
        if l.kind == "connected":
            after[l.index] = (host(tr.delta[l.index]), host(tr.fc[l.index]["wu"]),
                              host(tr.delta[l.index - 1]) if l.index else None)
    tr.backward(x, on_backward=snap)
    for l, p in zip(layers, params):
        d, wu, sd = after[l.index]
        d, sd = d.reshape(3, -1), None if sd is None else sd.reshape(3, -1)
        inp = host(x if l.index == 0 else tr.out[l.index - 1]).reshape(3, l.in_size)
        assert d.any()
        held(wu, *reference("TN", d, inp, np.zeros((l.filters, l.in_size))), f"layer {l.index} dW")
        if sd is not None:  # zeroed by the forward, written by this layer alone
            held(sd, *reference("NN", d, p.weights.reshape(l.filters, -1), np.zeros(sd.shape)),
                 f"layer {l.index} dX")
