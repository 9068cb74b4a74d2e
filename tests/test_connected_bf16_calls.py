"""connected_precision="bf16" changes the drivers' products and nothing else
(no GPU: tests/_driver_trace.Recorder stands in for TNNHip).

Against the default trace of the same net: no ``gemm`` (or
``gemmStridedBatched``) line is left in any phase; there are as many
``gemmBf16NTPacked`` (inference) or ``gemmBf16`` (training) lines as the default
issues products, a strided-batched call counting its batch; and with the
product lines taken out the traces are equal.  In inference the packed weights
are opaque to the recorder, so there the buffer numbering differs and the
method names are compared.
"""
import pytest
import torch

import _driver_trace as dt
from tensorium_amd import darknet as dn

MLP = ("[net]\nbatch=3\ninputs=20\n[connected]\noutput=33\nactivation=leaky\n"
       "[connected]\noutput=7\nactivation=linear\n[softmax]\n")
NETS = {"mlp": MLP,
        "lstm": dn.lstm_cfg(batch=4, time_steps=2, inputs=3, hidden=5, layers=1, bn=False),
        "rnn": dn.rnn_cfg(batch=4, time_steps=2, inputs=3, hidden=5, layers=1, bn=False)}
FP32 = ("gemm", "gemmStridedBatched")


def _trace(cfg, train, fused, precision):
    net = dn.Network(dn.parse_cfg(cfg), rnn=True)
    params = dn.random_params(net, seed=11)
    base = dn.HipDarknetTrain if train else dn.HipDarknet
    rec = dt.Recorder()
    rec.phase("build")
    model = type(base.__name__, (base,), {"device": "cpu"})(
        rec, net, params, torch, lstm_fused=fused, rnn_fused=fused, connected_precision=precision)
    x = torch.zeros(net.batch, net.inputs)
    rec.register(x)
    rec.register(vars(model))
    rec.phase("forward")
    if not train:
        model.forward(x)
        return rec.phases
    model.forward(x, torch.zeros(net.batch, net.layers[-1].out_size))
    rec.phase("backward")
    model.backward(x)
    rec.phase("update")
    model.update(0.01, 0.9, 0.0005)
    return rec.phases


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", NETS)
def test_only_the_products_change(name, train, fused):
    ref, got = (_trace(NETS[name], train, fused, p) for p in ("fp32", "bf16"))
    new = "gemmBf16" if train else "gemmBf16NTPacked"
    assert ref["build"] == [] and (got["build"] == []) == train
    assert all(l.split()[0] == "gemmBf16Pack" for l in got["build"])
    for phase in ref:
        if phase == "build":
            continue
        split = lambda ls: ([l.split() for l in ls if l.split()[0] in FP32 + (new,)],  # noqa: E731
                            [l if train else l.split()[0] for l in ls
                             if l.split()[0] not in FP32 + (new,)])
        (rp, rest), (gp, grest) = split(ref[phase]), split(got[phase])
        products = sum(int(p[-1]) if p[0] == "gemmStridedBatched" else 1 for p in rp)
        assert [p[0] for p in gp] == [new] * products, phase
        assert grest == rest, phase
    assert sum(len(ref[p]) for p in ("forward", "backward") if p in ref) > 0
    if not train:  # one pack a (sub-)layer, as many as the parameter blocks
        net = dn.Network(dn.parse_cfg(NETS[name]), rnn=True)
        assert len(got["build"]) == len(net.param_layers())
