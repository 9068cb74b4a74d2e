"""Networks that end in [avgpool] through HipDarknet / HipDarknetTrain against
tests/_avgpool_oracle.py's AvgRefNet, bit for bit:

* darknet19_cfg(96, batch 2, 10 classes): the final plane is 3x3 = 9, one
  block of eight plus a tail; darknet53_cfg(64, batch 2, 10 classes): the
  final plane is 2x2, tail only, feeding the connected layer — every layer's
  inference output;
* a cut-down residual classifier (conv, conv/2, 1x1, 3x3, shortcut, avgpool
  over 36, connected, softmax), the darknet19 tail (1x1 linear conv without
  batch norm, avgpool over 9, softmax: the pool directly under the loss) and
  a network whose first layer is the pool: two forward(truth) / backward /
  update steps, every output, delta, parameter, update buffer, rolling
  statistic and the cost;
* export_params() after the two steps against the checker's state, and the
  .weights file written from it run by HipDarknet against the checker's
  inference."""
import numpy as np
import pytest

from tensorium_amd import darknet as dn

from _avgpool_oracle import AvgRefNet
from test_gpu_classifier_net import DECAY, LR, MOM, mismatches, snapshot

pytestmark = pytest.mark.gpu

CLASSES = 10


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def bn_conv(f, k, s=1, act="leaky", bn=1):
    return (f"[convolutional]\nbatch_normalize={bn}\nfilters={f}\nsize={k}\nstride={s}\npad=1\n"
            f"activation={act}\n")


def net_head(B, c, h, w):
    return f"[net]\nbatch={B}\nwidth={w}\nheight={h}\nchannels={c}\n"


RESIDUAL = (net_head(4, 3, 12, 12) + bn_conv(8, 3) + bn_conv(16, 3, 2) + bn_conv(8, 1)
            + bn_conv(16, 3) + "[shortcut]\nfrom=-3\nactivation=linear\n[avgpool]\n"
            f"[connected]\noutput={CLASSES}\nactivation=linear\n[softmax]\n")
TAIL19 = (net_head(4, 3, 6, 6) + bn_conv(8, 3, 2) + bn_conv(CLASSES, 1, act="linear", bn=0)
          + "[avgpool]\n[softmax]\ngroups=1\n")
POOL_FIRST = (net_head(4, 6, 3, 5) + f"[avgpool]\n[connected]\noutput={CLASSES}\n"
              "activation=linear\n[softmax]\n")


def inputs(cfg, seed):
    net = dn.Network(dn.parse_cfg(cfg))
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (net.batch, net.c, net.h, net.w)).astype(np.float32)
    truth = np.zeros((net.batch, CLASSES), np.float32)
    truth[np.arange(net.batch), rng.integers(0, CLASSES, net.batch)] = 1
    return net, dn.random_params(net, seed=seed), x, truth


# ---- inference ----------------------------------------------------------------------

@pytest.mark.parametrize("builder,size,pool,plane", [(dn.darknet19_cfg, 96, 24, 9),
                                                     (dn.darknet53_cfg, 64, 75, 4)])
def test_classifier_inference(hip, torch_cuda, ora, builder, size, pool, plane):
    T = torch_cuda
    net, params, x, _ = inputs(builder(size, batch=2, classes=CLASSES), 91)
    a = net.layers[pool]
    assert a.kind == "avgpool" and a.h * a.w == plane
    want = AvgRefNet(ora, net, params).infer(x)
    model = dn.HipDarknet(hip, net, params, T)
    outs = model.forward(T.from_numpy(x).cuda())
    hip.finish()
    bad = [(l.index, l.kind) for l, o, r in zip(net.layers, outs, want)
           if not np.array_equal(bits(o.cpu().numpy()), bits(r))]
    assert not bad, bad[:8]
    assert outs[pool].numel() == 2 * a.c
    assert np.allclose(outs[-1].cpu().numpy().reshape(2, CLASSES).sum(1), 1, atol=1e-5)


# ---- training -----------------------------------------------------------------------

def trained(ora, cfg, seed):
    """The network, its inputs, the checker's snapshots after the backward
    and after the update of each of two steps, and the checker itself."""
    net, params, x, truth = inputs(cfg, seed)
    ref = AvgRefNet(ora, net, params)
    snaps = []
    for _ in range(2):
        ref.forward(x, truth)
        ref.backward(x)
        after_backward = snapshot(ref)
        ref.update(LR, MOM, DECAY)
        snaps.append((after_backward, snapshot(ref)))
    return net, params, x, truth, snaps, ref


def two_steps(hip, T, data):
    net, params, x, truth, snaps, _ = data
    model = dn.HipDarknetTrain(hip, net, params, T)
    X, Tr = T.from_numpy(x).cuda(), T.from_numpy(truth).cuda()
    bad = []
    for s in range(2):
        model.forward(X, Tr)
        model.backward(X)
        hip.finish()
        bad += [(s, "backward") + b for b in mismatches(net, model, snaps[s][0])]
        model.update(LR, MOM, DECAY)
        hip.finish()
        bad += [(s, "update") + b for b in mismatches(net, model, snaps[s][1])]
    assert hip.pendingDw() == 0
    assert np.array_equal(bits(X.cpu().numpy()), bits(x)), "the network input was written"
    return model, bad


@pytest.fixture(scope="module")
def residual(ora):
    return trained(ora, RESIDUAL, 92)


def test_residual_classifier_two_training_steps(hip, torch_cuda, residual):
    net, snaps = residual[0], residual[4]
    assert [l.kind for l in net.layers[4:]] == ["shortcut", "avgpool", "connected", "softmax"]
    assert net.layers[5].h * net.layers[5].w == 36 and net.layers[4].inputs == (1,)
    model, bad = two_steps(hip, torch_cuda, residual)
    assert not bad, bad[:12]
    after = snaps[1][0]   # the gradient went through the pool and both shortcut branches
    assert after["cost"] > 0 and all(np.abs(after["delta"][i]).max() > 0 for i in (0, 1, 3, 4, 5))


def test_pool_directly_under_the_loss(hip, torch_cuda, ora):
    data = trained(ora, TAIL19, 93)
    net = data[0]
    assert [l.kind for l in net.layers] == ["convolutional", "convolutional", "avgpool", "softmax"]
    assert not net.layers[1].bn and net.layers[2].h * net.layers[2].w == 9
    model, bad = two_steps(hip, torch_cuda, data)
    assert not bad, bad[:12]
    assert model.conv[1]["bu"].abs().max().item() > 0


def test_pool_as_the_first_layer(hip, torch_cuda, ora):
    """No state.delta below layer 0: the pool's backward does nothing, and
    the input stays as it was (two_steps checks it)."""
    data = trained(ora, POOL_FIRST, 94)
    assert data[0].layers[0].kind == "avgpool"
    model, bad = two_steps(hip, torch_cuda, data)
    assert not bad, bad[:12]
    assert model.delta[0].abs().max().item() > 0


def test_export_params_and_the_written_file(hip, torch_cuda, ora, residual, tmp_path):
    T = torch_cuda
    net, params, x, _, _, ref = residual
    model, bad = two_steps(hip, T, residual)
    assert not bad, bad[:12]
    got = model.export_params()
    assert len(got) == len(net.param_layers()) == 5
    names = dict(biases="b", weights="w", scales="scales", rolling_mean="rm", rolling_var="rv")
    for l, p, p0 in zip(net.param_layers(), got, params):
        st = ref.st[l.index]
        for field, key in names.items():
            a = getattr(p, field)
            if key not in st:
                assert a is None, (l.index, field)
                continue
            assert a.dtype == np.float32 and a.shape == getattr(p0, field).shape
            assert np.array_equal(bits(a), bits(st[key])), (l.index, field)
        assert not np.array_equal(p.weights, p0.weights)   # trained, not the initial ones
    path = tmp_path / "trained.weights"
    dn.write_weights(path, net, got)
    loaded, _ = dn.load_weights(path, net)
    want = ref.infer(x)
    outs = dn.HipDarknet(hip, net, loaded, T).forward(T.from_numpy(x).cuda())
    hip.finish()
    bad = [(l.index, l.kind) for l, o, r in zip(net.layers, outs, want)
           if not np.array_equal(bits(o.cpu().numpy()), bits(r))]
    assert not bad, bad
