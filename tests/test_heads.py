"""CPU checks for dropout / the loss heads and the classifier layer kinds:
the known answers of the reference's xorshift64* dropout generator, the
planner's five new sections (shapes, defaults, refusals), the three generated
sample networks against nmodels.pas, the .weights layout with connected
layers, and that conv-only networks draw and write exactly what a walk over
the convolutions alone gives."""
import struct

import numpy as np
import pytest

from tensorium_amd import darknet as dn
from tensorium_amd._abi import ACT

import _heads_oracle as ho
from _classifier_oracle import RefNet

NET = "[net]\nbatch=2\nwidth=4\nheight=4\nchannels=3\n"


def plan(body, head=NET, batch=None):
    return dn.Network(dn.parse_cfg(head + body), batch)


# ---- the generator ----------------------------------------------------------

KNOWN = {1234567: ([207249728, 57982620, 149003193, 105806038],
                   [0.7720654, 0.21600209, 0.5550802, 0.3941582]),
         0: ([0, 158129437, 47823418, 205952855], None)}


@pytest.mark.parametrize("seed", sorted(KNOWN))
def test_known_answers(seed):
    r, rnd = KNOWN[seed]
    assert [ho.xorshift_r(seed, i) for i in range(4)] == r
    assert ho.dropout_r(seed, 4).tolist() == r
    got = ho.dropout_rnd(seed, 4)
    assert got.dtype == np.float32
    # float(r) rounded to nearest even, then an exact division by 2^28
    want = np.array([np.float32(v) for v in r], np.float32) / np.float32(2 ** 28)
    assert np.array_equal(got, want)
    if rnd is not None:
        assert np.array_equal(got, np.array(rnd, np.float32))
    else:
        assert got[0] == 0.0


def test_seed_zero_drops_element_zero_for_any_positive_probability():
    src = np.full(4, 3.0, np.float32)
    _, dst = ho.dropout_forward(0, 1e-30, 1.0, src)
    assert dst[0] == 0.0 and np.all(dst[1:] == 3.0)
    _, dst = ho.dropout_forward(0, 0.0, 1.0, src)   # rnd == 0 < 0 is false: kept
    assert np.all(dst == 3.0)


def test_seed_plus_index_is_a_64_bit_sum():
    """0xFFFFFFFF + 1 is 0x100000000, not 0: the vector and the scalar
    statement agree across the 2^32 boundary and differ from a wrapped sum."""
    seed = 0xFFFFFFFF
    r = ho.dropout_r(seed, 3).tolist()
    assert r == [ho.xorshift_r(seed, i) for i in range(3)]
    x = 0x100000000                                   # seed + 1, unwrapped
    x ^= x >> 12
    x ^= (x << 25) & (2 ** 64 - 1)
    x ^= x >> 27
    assert r[1] == (x * 0x2545F4914F6CDD1D) % 2 ** 64 % 2 ** 28
    assert r[1] != ho.xorshift_r(0, 0) and r[2] != ho.xorshift_r(0, 1)
    # far indexes: an index past 2^32 on top of the largest seed
    assert ho.dropout_r(seed, 2, start=2 ** 33).tolist() == [
        ho.xorshift_r(seed, 2 ** 33), ho.xorshift_r(seed, 2 ** 33 + 1)]


def test_conversion_rounds_to_nearest_even():
    r = ho.dropout_r(1234567, 4096)
    assert np.mean(r >= 2 ** 24) > 0.9                # most values need more than 24 bits
    inexact = r.astype(np.float32).astype(np.uint64) != r
    assert 0.7 < inexact.mean() < 0.9                 # about 81 %
    rnd = ho.dropout_rnd(1234567, 4096)
    assert rnd.min() >= 0.0 and rnd.max() <= 1.0


def test_dropped_is_positive_zero_and_kept_is_one_multiply():
    src = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-42, -3.5, 2.0, 7.0], np.float32)
    rnd, dst = ho.dropout_forward(1234567, 0.5, 2.0, src)
    drop = rnd < np.float32(0.5)
    assert drop.any() and (~drop).any()
    assert np.all(dst[drop].view(np.uint32) == 0)     # +0.0f whatever src held
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.array_equal(dst[~drop].view(np.uint32), (src[~drop] * np.float32(2)).view(np.uint32))
    back = ho.dropout_backward(0.5, 2.0, src, rnd)
    assert np.array_equal(back.view(np.uint32), dst.view(np.uint32))


def test_loss_heads_oracle():
    p = np.array([0.0, 1.0, 5e-7, 1 - 5e-8, 0.25, 0.9], np.float32)
    t = np.array([1.0, 0.0, 0.3, 1.0, 0.0, 0.3], np.float32)
    d, e = ho.cross_entropy_logistic(p, t)
    assert np.array_equal(d, t - p)
    eps = float(np.float32(1e-6))
    assert e[0] == np.float32(-np.log(eps))           # t = 1, p clamped to eps
    assert e[1] == np.float32(-np.log(eps))           # t = 0, 1 - p clamped
    a, b = np.float64(np.float32(0.9)), np.float64(np.float32(1) - np.float32(0.9))
    t3, u3 = np.float64(np.float32(0.3)), np.float64(np.float32(1) - np.float32(0.3))
    assert e[5] == np.float32(-t3 * np.log(a) - u3 * np.log(b))
    d2, e2 = ho.cost_l2(p, t)
    assert np.array_equal(d2, t - p) and np.array_equal(e2, (t - p) * (t - p))


# ---- planner ------------------------------------------------------------------

def test_connected_defaults_and_shapes():
    net = plan("[connected]\n[conn]\noutput=7\nactivation=linear\nbatch_normalize=1\n")
    a, b = net.layers
    assert (a.kind, a.in_size, a.out_c, a.out_h, a.out_w) == ("connected", 48, 1, 1, 1)
    assert a.activation == ACT["RELU"] and not a.bn and a.filters == 1
    assert (b.kind, b.in_size, b.out_size, b.bn, b.activation) == ("connected", 1, 7, True,
                                                                    ACT["LINEAR"])
    assert net.param_layers() == [a, b] and net.convs() == []


def test_dropout_defaults_scale_and_shape():
    net = plan("[dropout]\n[dropout]\nprobability=0.5\n[dropout]\nprobability=0.999\n")
    a, b, c = net.layers
    assert (a.out_c, a.out_h, a.out_w) == (3, 4, 4)
    assert np.float32(a.probability) == np.float32(0.2)
    assert a.scale == float(np.float32(1.0 / (1.0 - float(np.float32(0.2)))))
    assert a.scale == float(ho.dropout_scale(0.2)) == 1.25
    assert b.scale == 2.0
    assert c.scale == float(ho.dropout_scale(0.999))
    assert net.param_layers() == []


def test_softmax_cost_logistic_defaults():
    net = plan("[connected]\noutput=12\n[softmax]\n[soft]\ngroups=3\ntemperature=2\nnoloss=1\n"
               "[cost]\n[cost]\ntype=L2\nscale=0.5\n[logistic]\n")
    _, s0, s1, c0, c1, lg = net.layers
    assert (s0.kind, s0.groups, s0.temperature, s0.noloss, s0.out_size) == ("softmax", 1, 1.0,
                                                                            False, 12)
    assert (s1.groups, s1.temperature, s1.noloss) == (3, 2.0, True)
    assert (c0.kind, c0.scale, c0.out_size) == ("cost", 1.0, 12) and c1.scale == 0.5
    assert (lg.kind, lg.activation, lg.out_size) == ("logistic", ACT["LOGISTIC"], 12)


@pytest.mark.parametrize("body,what", [
    ("[dropout]\nprobability=1\n", "below one"),
    ("[dropout]\nprobability=1.5\n", "below one"),
    ("[dropout]\ndropblock=1\n", "dropblock"),
    ("[softmax]\ntree=imagenet.tree\n", "tree"),
    ("[cost]\ntype=smooth\n", "type"),
    ("[cost]\ntype=masked\n", "type"),
    ("[connected]\noutput=4\n[convolutional]\nfilters=2\nsize=1\n", "after a \\[connected\\]"),
    ("[connected]\noutput=4\n[maxpool]\nsize=2\nstride=2\n", "after a \\[connected\\]"),
    ("[connected]\noutput=4\n[local_avgpool]\nsize=2\nstride=2\n", "after a \\[connected\\]"),
    ("[connected]\noutput=4\n[upsample]\n", "after a \\[connected\\]"),
    ("[connected]\noutput=4\n[shortcut]\nfrom=-1\n", "after a \\[connected\\]"),
    ("[connected]\noutput=4\n[route]\nlayers=-1\n", "after a \\[connected\\]"),
    ("[connected]\noutput=4\n[dropout]\n[yolo]\nmask=0\nclasses=0\n", "after a \\[connected\\]"),
])
def test_refusals(body, what):
    with pytest.raises(ValueError, match=what):
        plan(body)


def test_image_layers_after_dropout_keep_their_shape():
    net = plan("[dropout]\n[convolutional]\nfilters=5\nsize=3\npad=1\n[dropout]\n"
               "[maxpool]\nsize=2\nstride=2\npadding=0\n")
    assert [(l.kind, l.out_c, l.out_h, l.out_w) for l in net.layers] == [
        ("dropout", 3, 4, 4), ("convolutional", 5, 4, 4), ("dropout", 5, 4, 4),
        ("maxpool", 5, 2, 2)]


# ---- the sample networks (nmodels.pas) ---------------------------------------------

def shapes(cfg):
    net = dn.Network(dn.parse_cfg(cfg))
    return net, [(l.kind, l.out_c, l.out_h, l.out_w) for l in net.layers]


def test_cifar10_deep_cfg():
    net, got = shapes(dn.cifar10_deep_cfg(32))
    C, M, D, F = "convolutional", "maxpool", "dropout", "connected"
    assert got == [(C, 32, 32, 32), (C, 32, 32, 32), (M, 32, 16, 16),
                   (C, 64, 16, 16), (C, 64, 16, 16), (M, 64, 8, 8),
                   (C, 128, 8, 8), (C, 128, 8, 8), (M, 128, 4, 4),
                   (D, 128, 4, 4), (F, 1024, 1, 1), (D, 1024, 1, 1), (F, 10, 1, 1),
                   ("softmax", 10, 1, 1)]
    assert net.batch == 32 and (net.c, net.h, net.w) == (3, 32, 32)
    for l in net.convs():
        assert (l.size, l.stride, l.pad, l.bn, l.activation) == (3, 1, 1, True, ACT["RELU"])
    for l in net.layers:
        if l.kind == "maxpool":
            assert (l.size, l.stride_x, l.stride_y, l.pad) == (2, 2, 2, 0)
        if l.kind == "dropout":
            assert np.float32(l.probability) == np.float32(0.2)
    f1, f2 = net.layers[10], net.layers[12]
    assert (f1.in_size, f1.activation, f1.bn) == (4 * 4 * 128, ACT["RELU"], False)
    assert (f2.in_size, f2.activation, f2.bn) == (1024, ACT["LINEAR"], False)
    assert net.layers[9].out_size * 32 == 65536       # the layer scripts/heads_perf.py times


def test_lenet_cfgs():
    C, M, F = "convolutional", "maxpool", "connected"
    net, got = shapes(dn.lenet_cifar10_cfg(4))
    assert got == [(C, 6, 28, 28), (M, 6, 14, 14), (C, 12, 10, 10), (M, 12, 5, 5), (C, 120, 1, 1),
                   (F, 84, 1, 1), (F, 10, 1, 1), ("softmax", 10, 1, 1)]
    assert all((l.size, l.pad, l.bn, l.activation) == (5, 0, True, ACT["RELU"])
               for l in net.convs())
    assert (net.c, net.h, net.w) == (3, 32, 32)
    net, got = shapes(dn.lenet_mnist_cfg(4))
    assert got == [(C, 6, 28, 28), (M, 6, 14, 14), (C, 16, 10, 10), (M, 16, 5, 5), (C, 120, 1, 1),
                   (F, 84, 1, 1), (F, 10, 1, 1), ("softmax", 10, 1, 1)]
    assert [(l.size, l.pad, l.bn) for l in net.convs()] == [(5, 2, False), (5, 0, False),
                                                            (5, 0, False)]
    assert (net.c, net.h, net.w) == (1, 28, 28)
    assert [net.layers[i].activation for i in (5, 6)] == [ACT["RELU"], ACT["LINEAR"]]


# ---- parameters and the .weights layout ---------------------------------------------

MIXED = ("[convolutional]\nbatch_normalize=1\nfilters=4\nsize=3\npad=1\nactivation=relu\n"
         "[connected]\noutput=6\nbatch_normalize=1\n[dropout]\n[connected]\noutput=3\n"
         "activation=linear\n[softmax]\n")


def test_connected_initialisation_follows_the_constructor():
    net = plan(MIXED)
    ps = dn.random_params(net, seed=9)
    assert len(ps) == 3
    fc1, fc2 = ps[1], ps[2]
    s = np.float32(np.sqrt(2.0 / 64))
    assert fc1.weights.shape == (6, 64) and np.abs(fc1.weights).max() <= s
    assert np.abs(fc1.weights).max() > 0.8 * s
    assert not fc1.biases.any() and np.all(fc1.scales == 1)
    assert not fc1.rolling_mean.any() and not fc1.rolling_var.any()
    assert fc2.weights.shape == (3, 6) and fc2.scales is None and not fc2.biases.any()


def test_weights_round_trip_with_connected_layers(tmp_path):
    net = plan(MIXED)
    ps = dn.random_params(net, seed=10)
    rng = np.random.default_rng(1)
    for p in ps[1:]:   # make every array of the connected layers distinct
        p.biases[:] = rng.uniform(-1, 1, p.biases.size)
        if p.scales is not None:
            for t in (p.scales, p.rolling_mean, p.rolling_var):
                t[:] = rng.uniform(0.5, 1.5, t.size)
    path = tmp_path / "m.weights"
    dn.write_weights(path, net, ps, seen=77)
    got, seen = dn.load_weights(path, net)
    assert seen == 77 and len(got) == 3
    for a, b in zip(ps, got):
        for k in ("biases", "weights", "scales", "rolling_mean", "rolling_var"):
            x, y = getattr(a, k), getattr(b, k)
            assert (x is None) == (y is None), k
            assert x is None or np.array_equal(x, y), k
    # the layout: conv b, (s, m, v), W; connected b, W, (s, m, v); connected b, W
    raw = np.frombuffer(path.read_bytes(), "<f4", offset=20)
    order = [ps[0].biases, ps[0].scales, ps[0].rolling_mean, ps[0].rolling_var, ps[0].weights,
             ps[1].biases, ps[1].weights, ps[1].scales, ps[1].rolling_mean, ps[1].rolling_var,
             ps[2].biases, ps[2].weights]
    assert np.array_equal(raw, np.concatenate([t.ravel() for t in order]))
    with open(path, "r+b") as f:   # a file cut short
        f.truncate(path.stat().st_size - 4)
    with pytest.raises(ValueError, match="end of weights"):
        dn.load_weights(path, net)


@pytest.mark.parametrize("major,minor", [(1001, 0), (0, 1001)])
def test_transpose_flag_is_refused(tmp_path, major, minor):
    net = plan(MIXED)
    ps = dn.random_params(net, seed=10)
    with pytest.raises(ValueError, match="transpose"):
        dn.write_weights(tmp_path / "t.weights", net, ps, major=major, minor=minor)
    path = tmp_path / "u.weights"
    dn.write_weights(path, net, ps)
    data = bytearray(path.read_bytes())
    data[0:8] = struct.pack("<2i", major, minor)
    path.write_bytes(bytes(data))
    with pytest.raises(ValueError, match="transpose"):
        dn.load_weights(path, net)


def test_conv_only_networks_draw_and_write_what_they_did(tmp_path):
    """random_params / write_weights of yolov3-tiny against a walk over the
    convolutions alone (the draws and the byte layout before connected layers
    existed)."""
    net = dn.Network(dn.parse_cfg(dn.yolov3_tiny_cfg(64, batch=1, classes=2)))
    assert net.param_layers() == net.convs()
    ps = dn.random_params(net, seed=3)
    rng = np.random.default_rng(3)
    blob = [struct.pack("<3i", 0, 2, 0), struct.pack("<Q", 5)]
    for l, p in zip(net.convs(), ps):
        s = np.sqrt(2.0 / (l.size * l.size * l.c))
        w = rng.uniform(-s, s, (l.filters, l.c * l.size * l.size)).astype(np.float32)
        b = rng.uniform(-0.1, 0.1, l.filters).astype(np.float32)
        assert np.array_equal(p.weights, w) and np.array_equal(p.biases, b)
        blob.append(b.tobytes())
        if l.bn:
            for t, (lo, hi) in zip((p.scales, p.rolling_mean, p.rolling_var),
                                   ((0.5, 1.5), (-0.1, 0.1), (0.5, 2.0))):
                r = rng.uniform(lo, hi, l.filters).astype(np.float32)
                assert np.array_equal(t, r)
                blob.append(r.tobytes())
        else:
            assert p.scales is None
        blob.append(w.tobytes())
    path = tmp_path / "tiny.weights"
    dn.write_weights(path, net, ps, seen=5)
    assert path.read_bytes() == b"".join(blob)
    back, seen = dn.load_weights(path, net)
    assert seen == 5 and all(np.array_equal(a.weights, b.weights) for a, b in zip(ps, back))


# ---- the composed restatement against the oracle's connected train step ------------

@pytest.mark.parametrize("bn", [0, 1])
def test_restated_connected_net_equals_the_oracle_train_step(ora, bn):
    """tests/_classifier_oracle.py (the reference of the GPU network tests)
    composed call by call gives ora_mlp_train_step's buffer bit for bit."""
    from test_oracle_train import unpack
    widths, acts, B = [20, 9, 5], [ACT["RELU"], ACT["LINEAR"]], 6
    cfg = f"[net]\nbatch={B}\nwidth=5\nheight=4\nchannels=1\n" + "".join(
        f"[connected]\noutput={o}\nactivation={'relu' if a == ACT['RELU'] else 'linear'}\n"
        f"batch_normalize={bn}\n" for o, a in zip(widths[1:], acts)) + "[softmax]\n"
    net = dn.Network(dn.parse_cfg(cfg))
    buf = ora.mlp_init(widths, bn, B, seed=4)
    X, T = ora.mnist_batch(B, seed=4, classes=5, inputs=20)
    views = unpack(widths, bn, B, buf)
    params = [dn.ConvParams(v["b"].copy(), v["W"].reshape(o, -1).copy(),
                            *((v["scales"].copy(), v["rmean"].copy(), v["rvar"].copy())
                              if bn else ()))
              for v, o in zip(views, widths[1:])]
    ref = RefNet(ora, net, params)
    for _ in range(2):
        cost = ora.mlp_train_step(widths, acts, bn, B, X, T, 1e-2, 0.9, 1e-4, buf)
        ref.forward(X, T)
        ref.backward(X)
        ref.update(1e-2, 0.9, 1e-4)
        assert np.float32(ref.cost()) == np.float32(cost)
    names = {"W": "w", "b": "b", "dW": "wu", "db": "bu", "scales": "scales", "rmean": "rm",
             "rvar": "rv", "dscales": "su"}
    for i, v in enumerate(unpack(widths, bn, B, buf)):
        for k, a in v.items():
            assert np.array_equal(ref.st[i][names[k]].ravel(), a), (i, k)
