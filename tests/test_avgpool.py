"""[avgpool] in the layer plan, the darknet19 / darknet53 builders, their
.weights round trip, and the CPU checker's summation order (no GPU).

The order cases are worked by hand for vssum_avx2 (eight accumulators j, j+8,
...; a_j + a_(j+4); (s0+s1) + (s2+s3); the tail in index order; one division):
each plane holds 1e8, -1e8 and 1, whose sum is 1 exactly, and 1e8 + 1 rounds
to 1e8 in float32, so the result is 1/n when the order cancels the large pair
first and 0 when the 1 meets a large term first."""
from dataclasses import asdict

import numpy as np
import pytest

from tensorium_amd import darknet as dn

import _avgpool_oracle as ao

f32 = np.float32


def plan(cfg, **kw):
    return dn.Network(dn.parse_cfg(cfg), **kw)


def shape(l):
    return (l.out_c, l.out_h, l.out_w)


def test_darknet19_plan():
    net = plan(dn.darknet19_cfg(256))
    assert len(net.layers) == 26
    assert sum(l.kind == "convolutional" for l in net.layers) == 19
    assert shape(net.layers[23]) == (1000, 8, 8)
    head = net.layers[23]
    assert (head.size, head.bn, head.activation) == (1, False, dn.ACT["LINEAR"])
    a = net.layers[24]
    assert a.kind == "avgpool" and (a.c, a.h, a.w) == (1000, 8, 8) and shape(a) == (1000, 1, 1)
    assert net.layers[25].kind == "softmax" and net.layers[25].groups == 1
    # the public structure: filters and sizes of the 19 convolutions
    want = [(32, 3), (64, 3), (128, 3), (64, 1), (128, 3), (256, 3), (128, 1), (256, 3),
            (512, 3), (256, 1), (512, 3), (256, 1), (512, 3),
            (1024, 3), (512, 1), (1024, 3), (512, 1), (1024, 3), (1000, 1)]
    assert [(l.filters, l.size) for l in net.convs()] == want
    assert [l.index for l in net.layers if l.kind == "maxpool"] == [1, 3, 7, 11, 17]
    assert plan(dn.darknet19_cfg(96, batch=2, classes=10)).layers[24].in_size == 10 * 3 * 3


def test_darknet53_plan_shares_the_yolov3_backbone():
    net = plan(dn.darknet53_cfg(256))
    assert len(net.layers) == 78
    assert shape(net.layers[74]) == (1024, 8, 8)
    assert [l.kind for l in net.layers[75:]] == ["avgpool", "connected", "softmax"]
    assert shape(net.layers[75]) == (1024, 1, 1)
    assert net.layers[76].in_size == 1024 and net.layers[76].filters == 1000
    assert net.layers[76].activation == dn.ACT["LINEAR"]
    kinds = [l.kind for l in net.layers[:75]]
    assert kinds.count("convolutional") == 52 and kinds.count("shortcut") == 23
    yolo = plan(dn.yolov3_cfg(256))
    for a, b in zip(net.layers[:75], yolo.layers[:75]):
        assert asdict(a) == asdict(b), a.index


def test_avg_alias_and_what_may_follow():
    head = "[net]\nbatch=2\nwidth=6\nheight=5\nchannels=3\n"
    for name in ("avgpool", "avg"):
        net = plan(head + f"[{name}]\n[convolutional]\nfilters=4\nsize=1\nactivation=linear\n"
                   "[connected]\noutput=7\nactivation=linear\n")
        a, c, f = net.layers
        assert a.kind == "avgpool" and (a.c, a.h, a.w) == (3, 5, 6) and shape(a) == (3, 1, 1)
        assert (c.c, c.h, c.w) == (3, 1, 1) and shape(c) == (4, 1, 1)
        assert f.in_size == 4


@pytest.mark.parametrize("name", ["avgpool", "avg"])
def test_refusals(name):
    img = "[net]\nbatch=2\nwidth=4\nheight=4\nchannels=1\n"
    for before in ("[connected]\noutput=16\n", "[lstm]\noutput=16\n"):
        with pytest.raises(ValueError, match="refused"):
            plan(img + before + f"[{name}]\n")
    with pytest.raises(ValueError, match="refused"):
        plan(img + f"[rnn]\noutput=16\nhidden=8\n[{name}]\n", rnn=True)
    with pytest.raises(ValueError, match="refused"):   # the reference's stale-shape case
        plan(f"[net]\nbatch=2\ninputs=9\n[{name}]\n")
    with pytest.raises(ValueError, match="Layer before avgpool layer must output image"):
        plan("[net]\nbatch=2\nwidth=4\nheight=4\nchannels=3\n[convolutional]\nfilters=0\n"
             f"size=1\n[{name}]\n")


@pytest.mark.parametrize("builder", [dn.darknet19_cfg, dn.darknet53_cfg])
def test_weights_round_trip(builder, tmp_path):
    net = plan(builder(64, classes=10))
    params = dn.random_params(net, seed=5)
    assert len(params) == len(net.param_layers())
    path = tmp_path / "net.weights"
    dn.write_weights(path, net, params, seen=77)
    back, seen = dn.load_weights(path, net)
    assert seen == 77 and len(back) == len(params)
    for l, a, b in zip(net.param_layers(), params, back):
        for k in ("biases", "weights", "scales", "rolling_mean", "rolling_var"):
            x, y = getattr(a, k), getattr(b, k)
            assert (x is None) == (y is None) == (not l.bn and k not in ("biases", "weights"))
            if x is not None:
                assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))


def _one(ora, vals):
    x = np.array(vals, f32)
    return ao.forward(ora, x, 1, x.size)[0], f32(np.mean(x.astype(np.float64)))


def test_the_checker_tells_orders_apart(ora):
    z = [0.0] * 5
    # lanes 0 and 1 cancel in (s0+s1), the 1 waits in s2: the exact mean
    got, mean = _one(ora, [1e8, -1e8, 1] + z)
    assert got == mean == f32(0.125)
    # the 1 is s1 and meets 1e8 in (s0+s1): lost
    got, mean = _one(ora, [1e8, 1, -1e8] + z)
    assert got == 0 and mean == f32(0.125)
    # the 1 is a_4 and meets a_0 = 1e8 in the fold, which a sum in index order
    # (1e8 + 0 - 1e8 + 0 + 1) would keep
    got, mean = _one(ora, [1e8, 0, -1e8, 0, 1, 0, 0, 0])
    assert got == 0 and mean == f32(0.125)
    # a second block: accumulator 0 adds 1e8 then -1e8, accumulator 1 keeps the 1
    got, mean = _one(ora, [1e8, 1] + [0.0] * 6 + [-1e8] + [0.0] * 7)
    assert got == mean == f32(1 / 16)
    # the tail comes after the folds, in index order: 1e8 + (-1e8) + 1, against
    # 1e8 + 1 + (-1e8)
    got, mean = _one(ora, [1e8, -1e8] + [0.0] * 6 + [1])
    assert got == mean == f32(1) / f32(9)
    got, mean = _one(ora, [1e8, 1] + [0.0] * 6 + [-1e8])
    assert got == 0 and mean == f32(1) / f32(9)
    # below one block everything is tail: index order
    got, mean = _one(ora, [1e8, 1, -1e8])
    assert got == 0 and mean == f32(1) / f32(3)
    got, mean = _one(ora, [1e8, -1e8, 1])
    assert got == mean
    # the accumulators start at +0: a plane of -0.0 gives +0.0
    got, _ = _one(ora, [-0.0] * 11)
    assert got == 0 and not np.signbit(got)


def test_checker_backward_rounds_the_quotient_once():
    sd = np.array([1.0, -0.0, 3.0, 1e-8, 0.0, 2.0], f32)
    d = np.array([1.0, 0.0], f32)
    ao.backward(sd, d, 2, 3)
    q = f32(1) / f32(3)
    assert np.array_equal(sd[:3], np.array([f32(1) + q, f32(-0.0) + q, f32(3) + q], f32))
    assert np.array_equal(sd[3:].view(np.uint32), np.array([1e-8, 0.0, 2.0], f32).view(np.uint32))
    # -0.0 + 0.0 = +0.0: an add is made even where the quotient is zero
    sd = np.array([-0.0], f32)
    ao.backward(sd, np.array([0.0], f32), 1, 1)
    assert not np.signbit(sd[0])


def test_entry_points_declared_and_refuse_a_null_context(hiplib):
    from tensorium_amd import _abi
    for name in ("tns_pool_global_avg_forward", "tns_pool_global_avg_backward"):
        assert name in _abi.PROTOTYPES and name in _abi.header_symbols()
        assert getattr(hiplib, name)(None, 1, 1, None, None) == 1
        assert b"null tns_ctx" in hiplib.tns_last_error()
        hiplib.tns_clear_error()
    assert hiplib.tns_abi_version() == 1
