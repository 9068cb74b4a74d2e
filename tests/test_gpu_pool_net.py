"""Darknet networks with pooling layers through the HIP backend, bit-exact
against the restated passes of tests/_pool_oracle.py: yolov3-tiny (inference
and one training pass on the pipelined and the joined backward schedule), an
SPP block (three stride-1 pools of 5, 9 and 13 over one tensor, concatenated),
a net with local-average pools, one of them the first layer,
and the pipelined schedule across a pool's backward: it reads its own delta
and indexes and writes the layer below's delta, none of them a pending dW's
operand, so the dW products stay on the side stream."""
import numpy as np
import pytest

from tensorium_amd import darknet as dn

from _pool_oracle import infer_pass, train_pass

pytestmark = pytest.mark.gpu

CONV = ("[convolutional]\nbatch_normalize=1\nfilters={f}\nsize={k}\nstride=1\npad=1\n"
        "activation=leaky\n")


def _compare(net, model, outs, deltas, state, indexes):
    """test_gpu_train_net._compare, plus every maxpool's stored indexes."""
    for l in net.layers:
        i = l.index
        assert np.array_equal(model.out[i].cpu().numpy(), outs[i]), f"output {i} ({l.kind})"
        assert np.array_equal(model.delta[i].cpu().numpy(), deltas[i]), f"delta {i} ({l.kind})"
        if l.kind == "maxpool":
            assert np.array_equal(model.indexes[i].cpu().numpy(), indexes[i].ravel()), \
                f"indexes {i}"
        if l.kind != "convolutional":
            continue
        st, rs = model.conv[i], state[i]
        assert np.array_equal(st["wu"].cpu().numpy(), rs["wu"]), f"weight_updates {i}"
        if l.bn:
            for k in ("su", "md", "vd", "mean", "var", "rm", "rv"):
                assert np.array_equal(st[k].cpu().numpy(), rs[k]), f"{k} {i}"
        else:
            assert np.array_equal(st["bu"].cpu().numpy(), rs["bu"]), f"bias_updates {i}"


def _train(hip, torch, net, params, x, yd, mode, seed_delta=None, on_backward=None):
    model = dn.HipDarknetTrain(hip, net, params, torch)
    X = torch.from_numpy(x).cuda()
    try:
        hip.setBwdOverlap(mode)
        model.forward(X)
        model.set_yolo_deltas([torch.from_numpy(d).cuda() for d in yd])
        for i, d in (seed_delta or {}).items():
            model.delta[i].copy_(torch.from_numpy(d).cuda())
        model.backward(X, on_backward)
        hip.finish()
    finally:
        hip.setBwdOverlap(True)
    return model


@pytest.fixture(scope="module")
def tiny(ora):
    """yolov3-tiny at 64 px, batch 2, 2 classes, and its reference passes
    (computed once, read only)."""
    net = dn.Network(dn.parse_cfg(dn.yolov3_tiny_cfg(64, batch=2, classes=2)))
    params = dn.random_params(net, seed=71)
    rng = np.random.default_rng(71)
    x = rng.uniform(0, 1, (2, 3, 64, 64)).astype(np.float32)
    yd = [rng.uniform(-0.1, 0.1, 2 * l.out_size).astype(np.float32)
          for l in net.layers if l.kind == "yolo"]
    return net, params, x, yd, infer_pass(ora, net, params, x), train_pass(ora, net, params, x, yd)


def test_yolov3_tiny_forward(hip, torch_cuda, tiny):
    net, params, x, _, ref, _ = tiny
    assert sum(l.kind == "maxpool" for l in net.layers) == 6
    model = dn.HipDarknet(hip, net, params, torch_cuda)
    outs = model.forward(torch_cuda.from_numpy(x).cuda())
    hip.finish()
    for l, o, r in zip(net.layers, outs, ref):
        assert np.array_equal(o.cpu().numpy(), r), (l.index, l.kind)


@pytest.mark.parametrize("mode", [2, 1])
def test_yolov3_tiny_train_pass(hip, torch_cuda, tiny, mode):
    net, params, x, yd, _, (outs, deltas, state, indexes) = tiny
    model = _train(hip, torch_cuda, net, params, x, yd, mode)
    assert hip.pendingDw() == 0
    _compare(net, model, outs, deltas, state, indexes)


@pytest.mark.parametrize("mode", [2, 1])
def test_spp_block_train_pass(hip, torch_cuda, ora, mode):
    """conv -> max 5/1 -> route -2 -> max 9/1 -> route -4 -> max 13/1 ->
    route -1,-3,-5,-6 -> conv at 13x13 (yolov3-spp's block): every window
    larger than half the plane, each input element under up to 169 windows."""
    pool = "[maxpool]\nstride=1\nsize={}\n"
    cfg = ("[net]\nbatch=2\nwidth=13\nheight=13\nchannels=4\n" + CONV.format(f=8, k=3) +
           pool.format(5) + "[route]\nlayers=-2\n" + pool.format(9) + "[route]\nlayers=-4\n" +
           pool.format(13) + "[route]\nlayers=-1,-3,-5,-6\n" + CONV.format(f=6, k=1))
    net = dn.Network(dn.parse_cfg(cfg))
    assert [(l.kind, l.out_c, l.out_h) for l in net.layers[5:]] == [
        ("maxpool", 8, 13), ("route", 32, 13), ("convolutional", 6, 13)]
    params = dn.random_params(net, seed=72)
    rng = np.random.default_rng(72)
    x = rng.uniform(0, 1, (2, 4, 13, 13)).astype(np.float32)
    top = {7: rng.uniform(-1, 1, 2 * net.layers[7].out_size).astype(np.float32)}
    outs, deltas, state, indexes = train_pass(ora, net, params, x, [], seed_delta=top)
    model = _train(hip, torch_cuda, net, params, x, [], mode, seed_delta=top)
    _compare(net, model, outs, deltas, state, indexes)


@pytest.mark.parametrize("mode", [2, 1])
def test_avgpool_net_and_pool_as_first_layer(hip, torch_cuda, ora, mode):
    """local_avgpool 2/2 as layer 0 (no state.delta: its backward does
    nothing) -> conv -> local_avgpool 3/1 (overlapping) -> maxpool 2/2 as the
    last layer, inference and one training pass."""
    cfg = ("[net]\nbatch=2\nwidth=18\nheight=14\nchannels=3\n[local_avgpool]\nsize=2\nstride=2\n" +
           CONV.format(f=8, k=3) + "[local_avgpool]\nsize=3\nstride=1\n[max]\nsize=2\nstride=2\n")
    net = dn.Network(dn.parse_cfg(cfg))
    assert [(l.kind, l.out_h, l.out_w) for l in net.layers] == [
        ("local_avgpool", 7, 9), ("convolutional", 7, 9), ("local_avgpool", 7, 9),
        ("maxpool", 4, 5)]
    params = dn.random_params(net, seed=74)
    rng = np.random.default_rng(74)
    x = rng.uniform(0, 1, (2, 3, 14, 18)).astype(np.float32)
    top = {3: rng.uniform(-1, 1, 2 * net.layers[3].out_size).astype(np.float32)}
    outs, deltas, state, indexes = train_pass(ora, net, params, x, [], seed_delta=top)
    model = _train(hip, torch_cuda, net, params, x, [], mode, seed_delta=top)
    _compare(net, model, outs, deltas, state, indexes)
    ref = infer_pass(ora, net, params, x)
    got = dn.HipDarknet(hip, net, params, torch_cuda).forward(torch_cuda.from_numpy(x).cuda())
    hip.finish()
    for l, o, r in zip(net.layers, got, ref):
        assert np.array_equal(o.cpu().numpy(), r), (l.index, l.kind)


def test_pool_backward_keeps_the_pipeline_running(hip, torch_cuda, ora):
    """conv -> maxpool -> conv -> conv on the pipelined schedule: the dW
    products pending before the pool's backward are still pending after it."""
    cfg = ("[net]\nbatch=2\nwidth=32\nheight=32\nchannels=16\n" + CONV.format(f=16, k=3) +
           "[maxpool]\nsize=2\nstride=2\n" + CONV.format(f=32, k=3) + CONV.format(f=16, k=1))
    net = dn.Network(dn.parse_cfg(cfg))
    params = dn.random_params(net, seed=73)
    rng = np.random.default_rng(73)
    x = rng.uniform(0, 1, (2, 16, 32, 32)).astype(np.float32)
    top = {3: rng.uniform(-1, 1, 2 * net.layers[3].out_size).astype(np.float32)}
    outs, deltas, state, indexes = train_pass(ora, net, params, x, [], seed_delta=top)
    seen = []
    model = _train(hip, torch_cuda, net, params, x, [], 2, seed_delta=top,
                   on_backward=lambda l: seen.append((l.kind, hip.pendingDw())))
    assert hip.pendingDw() == 0
    assert [k for k, _ in seen] == ["convolutional", "convolutional", "maxpool", "convolutional"]
    before, after = seen[1][1], seen[2][1]
    assert before >= 1, seen           # the conv above left its dW on the side stream
    assert after >= before, seen       # ... and the pool's backward did not join it
    _compare(net, model, outs, deltas, state, indexes)


@pytest.fixture(scope="module")
def wide(ora):
    """A 12 x 20 net (batch 2, 16 channels): conv 3x3/1 -> conv 3x3/2 -> conv
    1x1 -> conv 3x3/1 -> shortcut -3 -> upsample 2 -> route -1,0 -> conv 1x1,
    and its reference passes (computed once, read only).  Every plane is
    non-square; the stride-2 layer's 12 x 20 input gives 6 x 10."""
    conv = ("[convolutional]\nbatch_normalize=1\nfilters={f}\nsize={k}\nstride={s}\npad=1\n"
            "activation=leaky\n")
    cfg = ("[net]\nbatch=2\nwidth=20\nheight=12\nchannels=16\n" + conv.format(f=32, k=3, s=1) +
           conv.format(f=64, k=3, s=2) + conv.format(f=32, k=1, s=1) + conv.format(f=64, k=3, s=1) +
           "[shortcut]\nfrom=-3\nactivation=linear\n[upsample]\nstride=2\n[route]\nlayers=-1,0\n" +
           conv.format(f=24, k=1, s=1))
    net = dn.Network(dn.parse_cfg(cfg))
    assert [(l.kind, l.out_c, l.out_h, l.out_w) for l in net.layers] == [
        ("convolutional", 32, 12, 20), ("convolutional", 64, 6, 10), ("convolutional", 32, 6, 10),
        ("convolutional", 64, 6, 10), ("shortcut", 64, 6, 10), ("upsample", 64, 12, 20),
        ("route", 96, 12, 20), ("convolutional", 24, 12, 20)]
    params = dn.random_params(net, seed=75)
    rng = np.random.default_rng(75)
    x = rng.uniform(0, 1, (2, 16, 12, 20)).astype(np.float32)
    top = {7: rng.uniform(-1, 1, 2 * net.layers[7].out_size).astype(np.float32)}
    return (net, params, x, top, infer_pass(ora, net, params, x),
            train_pass(ora, net, params, x, [], seed_delta=top))


def test_nonsquare_net_forward(hip, torch_cuda, wide):
    net, params, x, _, ref, _ = wide
    got = dn.HipDarknet(hip, net, params, torch_cuda).forward(torch_cuda.from_numpy(x).cuda())
    hip.finish()
    for l, o, r in zip(net.layers, got, ref):
        assert np.array_equal(o.cpu().numpy(), r), (l.index, l.kind)


@pytest.mark.parametrize("mode", [2, 1])
def test_nonsquare_net_train_pass(hip, torch_cuda, wide, mode):
    net, params, x, top, _, (outs, deltas, state, indexes) = wide
    model = _train(hip, torch_cuda, net, params, x, [], mode, seed_delta=top)
    assert hip.pendingDw() == 0
    _compare(net, model, outs, deltas, state, indexes)
