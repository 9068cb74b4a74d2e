"""Classifier networks through HipDarknetTrain / HipDarknet, bit for bit:

* [connected] x n + [softmax] against the oracle's whole connected train step
  (ora.mlp_init / ora.mlp_train_step; the layer's bnMomentum 0.05 is the value
  ora_mlp_train_step uses, so nothing is passed through), three
  forward / backward / update steps, every parameter, update buffer and the
  cost;
* lenet_cifar10_cfg and cifar10_deep_cfg at batch 4, two training steps with
  fixed dropout seeds on the joined and the pipelined backward schedule,
  against tests/_classifier_oracle.py (composed from the oracle's restated
  calls, tests/_pool_oracle.py and tests/_heads_oracle.py): every layer's
  output, delta, rnd, update buffer, BN statistic and the parameters after
  each update;
* a [cost] and a [logistic] head on a two-layer connected net;
* inference through HipDarknet on cifar10_deep_cfg."""
import numpy as np
import pytest

from tensorium_amd import darknet as dn
from tensorium_amd._abi import ACT

from _classifier_oracle import RefNet
from test_oracle_train import unpack

pytestmark = pytest.mark.gpu

LR, MOM, DECAY = 1e-2, 0.9, 1e-4
ACT_NAME = {ACT["RELU"]: "relu", ACT["LINEAR"]: "linear", ACT["LOGISTIC"]: "logistic"}


def fc_cfg(widths, acts, bn, B, head="[softmax]\n"):
    body = "".join(f"[connected]\noutput={o}\nactivation={ACT_NAME[a]}\nbatch_normalize={bn}\n"
                   for o, a in zip(widths[1:], acts))
    return f"[net]\nbatch={B}\nwidth={widths[0]}\nheight=1\nchannels=1\n" + body + head


def params_of(widths, bn, B, buf):
    return [dn.ConvParams(v["b"].copy(), v["W"].reshape(o, -1).copy(),
                          *((v["scales"].copy(), v["rmean"].copy(), v["rvar"].copy())
                            if bn else ()))
            for v, o in zip(unpack(widths, bn, B, buf), widths[1:])]


NAMES = {"W": "w", "b": "b", "dW": "wu", "db": "bu", "scales": "scales", "rmean": "rm",
         "rvar": "rv", "dscales": "su"}


@pytest.mark.parametrize("widths,B,seed", [([784, 64, 64, 32, 32, 10], 32, 5),
                                           ([101, 37, 10], 20, 11)])
@pytest.mark.parametrize("bn", [0, 1])
def test_connected_net_against_the_oracle_train_step(hip, torch_cuda, ora, widths, B, seed, bn):
    T = torch_cuda
    acts = [ACT["RELU"]] * (len(widths) - 2) + [ACT["LINEAR"]]
    net = dn.Network(dn.parse_cfg(fc_cfg(widths, acts, bn, B)))
    buf = ora.mlp_init(widths, bn, B, seed=seed)
    X, Tr = ora.mnist_batch(B, seed=seed, classes=widths[-1], inputs=widths[0])
    model = dn.HipDarknetTrain(hip, net, params_of(widths, bn, B, buf), T)
    dX, dT = T.from_numpy(X).cuda(), T.from_numpy(Tr).cuda()
    bad = []
    for step in range(3):
        cost = ora.mlp_train_step(widths, acts, bn, B, X, Tr, LR, MOM, DECAY, buf)
        model.forward(dX, dT)
        model.backward(dX)
        model.update(LR, MOM, DECAY)
        hip.finish()
        if np.float32(model.cost()) != np.float32(cost):
            bad.append((step, "cost", model.cost(), cost))
        for i, v in enumerate(unpack(widths, bn, B, buf)):
            for k, a in v.items():
                g = model.fc[i][NAMES[k]].cpu().numpy().ravel()
                if not np.array_equal(g, a):
                    bad.append((step, i, k, int((g != a).sum())))
    assert not bad, bad


# ---- the sample networks ----------------------------------------------------------

STATE_KEYS = ("w", "b", "wu", "bu", "scales", "rm", "rv", "su", "mean", "var", "md", "vd", "x",
              "xn")


def snapshot(ref):
    cp = lambda a: np.array(a, np.float32, copy=True).ravel()  # noqa: E731
    return dict(out=[cp(o) for o in ref.out], delta=[cp(d) for d in ref.delta],
                rnd={i: cp(r) for i, r in ref.rnd.items()},
                idx={i: np.array(x).ravel() for i, x in ref.indexes.items()},
                st={i: {k: cp(v) for k, v in st.items()} for i, st in ref.st.items()},
                cost=ref.cost())


def mismatches(net, model, snap):
    bad = []

    def chk(name, got, want):
        g = got.cpu().numpy().ravel()
        if not np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                              want.view(np.uint32) if want.dtype == np.float32 else want):
            bad.append((name, int((g != want).sum())))

    for l in net.layers:
        i = l.index
        chk(f"output {i} {l.kind}", model.out[i], snap["out"][i])
        chk(f"delta {i} {l.kind}", model.delta[i], snap["delta"][i])
        if l.kind == "dropout":
            chk(f"rnd {i}", model.rnd[i], snap["rnd"][i])
        if l.kind == "maxpool":
            chk(f"indexes {i}", model.indexes[i], snap["idx"][i])
        st = model.conv.get(i) or model.fc.get(i)
        if st is not None:
            for k in STATE_KEYS:
                if k in st and k in snap["st"][i]:
                    chk(f"{k} {i} {l.kind}", st[k], snap["st"][i][k])
    if np.float32(model.cost()) != np.float32(snap["cost"]):
        bad.append(("cost", model.cost(), snap["cost"]))
    return bad


def sample(ora, cfg, seed):
    """The network, its inputs, and the reference's state after the backward
    and after the update of each of two steps (computed once, read only)."""
    net = dn.Network(dn.parse_cfg(cfg))
    B = net.batch
    params = dn.random_params(net, seed=seed)
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (B, net.c, net.h, net.w)).astype(np.float32)
    truth = np.zeros((B, 10), np.float32)
    truth[np.arange(B), rng.integers(0, 10, B)] = 1
    ndrop = sum(l.kind == "dropout" for l in net.layers)
    seeds = [[1234567 + 10 * s + k for k in range(ndrop)] for s in range(2)]
    ref = RefNet(ora, net, params)
    snaps = []
    for s in range(2):
        ref.forward(x, truth, seeds[s])
        ref.backward(x)
        after_backward = snapshot(ref)
        ref.update(LR, MOM, DECAY)
        snaps.append((after_backward, snapshot(ref)))
    return net, params, x, truth, seeds, snaps


@pytest.fixture(scope="module")
def lenet(ora):
    return sample(ora, dn.lenet_cifar10_cfg(4), 81)


@pytest.fixture(scope="module")
def deep(ora):
    return sample(ora, dn.cifar10_deep_cfg(4), 82)


def run_two_steps(hip, T, data, mode):
    net, params, x, truth, seeds, snaps = data
    model = dn.HipDarknetTrain(hip, net, params, T)
    X, Tr = T.from_numpy(x).cuda(), T.from_numpy(truth).cuda()
    bad = []
    try:
        hip.setBwdOverlap(mode)
        for s in range(2):
            model.forward(X, Tr, seeds[s])
            model.backward(X)
            hip.finish()
            bad += [(s, "backward") + b for b in mismatches(net, model, snaps[s][0])]
            model.update(LR, MOM, DECAY)
            hip.finish()
            bad += [(s, "update") + b for b in mismatches(net, model, snaps[s][1])]
    finally:
        hip.setBwdOverlap(True)
    assert hip.pendingDw() == 0
    assert np.array_equal(X.cpu().numpy(), x), "the network input was written"
    return model, bad


@pytest.mark.parametrize("mode", [1, 2])
def test_lenet_cifar10_two_training_steps(hip, torch_cuda, lenet, mode):
    model, bad = run_two_steps(hip, torch_cuda, lenet, mode)
    assert not bad, bad[:12]


@pytest.mark.parametrize("mode", [1, 2])
def test_cifar10_deep_two_training_steps(hip, torch_cuda, deep, mode):
    net = deep[0]
    model, bad = run_two_steps(hip, torch_cuda, deep, mode)
    assert not bad, bad[:12]
    for i in (9, 11):   # the dropout layers' buffers are the layer below's
        assert net.layers[i].kind == "dropout"
        assert model.out[i].data_ptr() == model.out[i - 1].data_ptr()
        assert model.delta[i].data_ptr() == model.delta[i - 1].data_ptr()
        r = model.rnd[i].cpu().numpy()
        o = model.out[i].cpu().numpy()
        assert np.all(o[r < np.float32(0.2)] == 0) and (r < np.float32(0.2)).any()


def test_lenet_mnist_two_training_steps(hip, torch_cuda, ora):
    """Convolutions without batch norm (bias_updates through convBackward)
    under connected layers, on the pipelined schedule."""
    data = sample(ora, dn.lenet_mnist_cfg(4), 84)
    assert not any(l.bn for l in data[0].layers)
    model, bad = run_two_steps(hip, torch_cuda, data, 2)
    assert not bad, bad[:12]
    assert model.conv[0]["bu"].abs().max().item() > 0


@pytest.mark.parametrize("head,scale", [("[cost]\n", 1.0), ("[cost]\ntype=L2\nscale=0.5\n", 0.5),
                                        ("[logistic]\n", None)])
@pytest.mark.parametrize("bn", [0, 1])
def test_cost_and_logistic_heads(hip, torch_cuda, ora, head, scale, bn):
    T = torch_cuda
    widths, B = [23, 17, 6], 5
    acts = [ACT["RELU"], ACT["LINEAR"]]
    net = dn.Network(dn.parse_cfg(fc_cfg(widths, acts, bn, B, head)))
    params = dn.random_params(net, seed=83)
    rng = np.random.default_rng(83)
    x = rng.uniform(-1, 1, (B, widths[0])).astype(np.float32)
    truth = rng.choice(np.array([0.0, 1.0, 0.3], np.float32), (B, widths[-1])).astype(np.float32)
    ref = RefNet(ora, net, params)
    ref.forward(x, truth)
    ref.backward(x)
    after_backward = snapshot(ref)
    ref.update(LR, MOM, DECAY)
    model = dn.HipDarknetTrain(hip, net, params, T)
    X = T.from_numpy(x).cuda()
    model.forward(X, T.from_numpy(truth).cuda())
    model.backward(X)
    hip.finish()
    bad = mismatches(net, model, after_backward)
    model.update(LR, MOM, DECAY)
    hip.finish()
    bad += mismatches(net, model, snapshot(ref))
    assert not bad, bad
    assert after_backward["cost"] > 0 and np.abs(after_backward["delta"][0]).max() > 0
    if scale is not None:
        assert net.layers[-1].scale == scale


def test_forward_without_truth_and_default_seeds(hip, torch_cuda, deep):
    """forward(x) stays valid: no loss, seeds drawn in [0, 2^28) from the
    generator seeded at construction — the same for the same seed."""
    T = torch_cuda
    net, params, x = deep[:3]
    X = T.from_numpy(x).cuda()
    rnds = []
    for seed in (7, 7, 8):
        model = dn.HipDarknetTrain(hip, net, params, T, seed=seed)
        model.forward(X)
        hip.finish()
        rnds.append(model.rnd[9].cpu().numpy())
        assert model.cost() == 0.0 and not model.delta[13].any()
    assert np.array_equal(rnds[0], rnds[1]) and not np.array_equal(rnds[0], rnds[2])
    with pytest.raises(ValueError, match="seeds"):
        model.forward(X, None, [1])


def test_cifar10_deep_inference(hip, torch_cuda, ora, deep):
    T = torch_cuda
    net, params, x = deep[:3]
    want = RefNet(ora, net, params).infer(x)
    model = dn.HipDarknet(hip, net, params, T)
    outs = model.forward(T.from_numpy(x).cuda())
    hip.finish()
    for l, o, r in zip(net.layers, outs, want):
        assert np.array_equal(o.cpu().numpy(), r), (l.index, l.kind)
    for i in (9, 11):   # dropout changes nothing: its output is the layer below's
        assert outs[i].data_ptr() == outs[i - 1].data_ptr()
    assert np.allclose(outs[-1].cpu().numpy().reshape(4, 10).sum(1), 1, atol=1e-5)
