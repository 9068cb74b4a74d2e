"""The lstm layer without a GPU: the planner (``[net]`` time_steps / inputs,
``[lstm]``), the .weights layout of its eight connected blocks, the CPU
restatement tests/_lstm_oracle.py against a textbook float64 LSTM, and the
Pascal / C declarations of the two fused gate entries."""
import re
import struct
from pathlib import Path

import numpy as np
import pytest

from tensorium_amd import darknet as dn

from _lstm_oracle import LstmRefNet

ROOT = Path(__file__).resolve().parents[1]


def plan(cfg, batch=None):
    return dn.Network(dn.parse_cfg(cfg), batch)


# ---- planner -------------------------------------------------------------------------

def test_lstm_cfg_shapes():
    net = plan(dn.lstm_cfg(batch=32, time_steps=16))
    assert (net.batch, net.time_steps, net.inputs) == (512, 16, 256)
    assert (net.h, net.w, net.c) == (0, 0, 0)
    assert [l.kind for l in net.layers] == ["lstm"] * 3 + ["connected", "softmax"]
    for l, i in zip(net.layers[:3], (256, 1024, 1024)):
        assert (l.in_size, l.out_c, l.out_h, l.out_w, l.filters, l.bn, l.steps) == (
            i, 1024, 1, 1, 1024, True, 16)
    fc = net.layers[3]
    assert (fc.in_size, fc.filters, fc.activation) == (1024, 256, dn.ACT["LINEAR"])
    assert net.layers[4].in_size == 256
    small = plan(dn.lstm_cfg(3, 2, inputs=7, hidden=5, layers=1, bn=False, cost=True))
    assert [l.kind for l in small.layers] == ["lstm", "connected", "softmax", "cost"]
    assert not small.layers[0].bn and small.batch == 6
    assert [l.kind for l in small.lstms()] == ["lstm"]


def test_batch_is_batch_times_time_steps_and_the_argument_replaces_the_product():
    cfg = dn.lstm_cfg(batch=5, time_steps=4, inputs=7, hidden=5, layers=1)
    assert plan(cfg).batch == 20
    assert plan(cfg, batch=8).batch == 8            # ABatch replaces mini_batch * timeSteps
    assert plan(cfg, batch=8).time_steps == 4
    # nothing changes without time_steps
    img = "[net]\nbatch=6\nwidth=4\nheight=4\nchannels=2\n[connected]\noutput=3\n"
    net = plan(img)
    assert (net.batch, net.time_steps, net.inputs) == (6, 1, 32)
    assert plan("[net]\nbatch=6\ntime_steps=3\nwidth=4\nheight=4\nchannels=2\n"
                "[lstm]\noutput=3\n").layers[0].in_size == 32


def test_lstm_options():
    net = plan("[net]\nbatch=2\ninputs=9\n[lstm]\n[lstm]\noutput=4\nbatch_normalize=1\n")
    a, b = net.layers
    assert (a.filters, a.bn, a.in_size, a.steps) == (1, False, 9, 1)
    assert (b.filters, b.bn, b.in_size) == (4, True, 1)


@pytest.mark.parametrize("kind", ["convolutional", "maxpool", "upsample", "shortcut"])
def test_an_image_kind_in_an_inputs_net_is_refused(kind):
    opts = {"convolutional": "filters=2\nsize=1\n", "maxpool": "size=2\nstride=2\n",
            "upsample": "stride=2\n", "shortcut": "from=-1\n"}[kind]
    with pytest.raises(ValueError, match="refused"):
        plan(f"[net]\nbatch=2\ninputs=9\n[{kind}]\n{opts}")
    with pytest.raises(ValueError, match="refused"):   # and after an [lstm] on an image
        plan(f"[net]\nbatch=2\nwidth=4\nheight=4\nchannels=1\n[lstm]\noutput=16\n[{kind}]\n{opts}")


def test_refusals():
    cfg = dn.lstm_cfg(batch=5, time_steps=4, inputs=7, hidden=5, layers=1)
    with pytest.raises(ValueError, match="time_steps"):
        plan(cfg, batch=10)                          # the reference truncates 10 div 4
    for kind in ("rnn", "gru", "crnn", "conv_lstm"):
        with pytest.raises(ValueError, match="not yet implemented"):
            plan(f"[net]\nbatch=2\ninputs=9\n[{kind}]\noutput=4\n")
    with pytest.raises(ValueError, match="inputs"):
        plan("[net]\nbatch=2\n[lstm]\noutput=4\n")


# ---- weights --------------------------------------------------------------------------

@pytest.mark.parametrize("bn", [False, True])
def test_weights_round_trip_and_block_offsets(tmp_path, bn):
    I, O = 7, 5
    net = plan(dn.lstm_cfg(2, 3, inputs=I, hidden=O, layers=2, bn=bn))
    blocks = net.param_layers()
    assert [b.gate for b in blocks] == list(dn.LSTM_GATES) * 2 + [""]
    assert [b.index for b in blocks] == [0] * 8 + [1] * 8 + [2]
    assert [b.in_size for b in blocks[:8]] == [O] * 4 + [I] * 4
    assert [b.in_size for b in blocks[8:16]] == [O] * 8
    params = dn.random_params(net, seed=9)
    rng = np.random.default_rng(1)
    for p in params:   # (biases are drawn 0, scales 1: make every array distinct)
        p.biases[:] = rng.uniform(-1, 1, p.biases.size)
        if p.scales is not None:
            for a in (p.scales, p.rolling_mean, p.rolling_var):
                a[:] = rng.uniform(0.5, 1.5, a.size)
    path = tmp_path / "lstm.weights"
    dn.write_weights(path, net, params, seen=77)
    data = path.read_bytes()
    off = 20                                        # 3 int32 + uint64 seen
    for b, p in zip(blocks, params):                # loadConnectedWeights' layout, block by block
        assert p.weights.shape == (b.filters, b.in_size)
        parts = [p.biases, p.weights.ravel()] + ([p.scales, p.rolling_mean, p.rolling_var]
                                                 if b.bn else [])
        for a in parts:
            got = np.frombuffer(data, "<f4", a.size, off)
            assert np.array_equal(got, a), (b.index, b.gate, off)
            off += 4 * a.size
    assert off == len(data)
    loaded, seen = dn.load_weights(path, net)
    assert seen == 77 and len(loaded) == len(params)
    for p, q in zip(params, loaded):
        for k in ("biases", "weights", "scales", "rolling_mean", "rolling_var"):
            a, b = getattr(p, k), getattr(q, k)
            assert (a is None and b is None) or np.array_equal(a, b), k
    path.write_bytes(data[:-4])
    with pytest.raises(ValueError, match="end of weights"):
        dn.load_weights(path, net)


def test_draw_is_the_connected_layers():
    net = plan(dn.lstm_cfg(2, 3, inputs=7, hidden=5, layers=1, bn=True))
    ps = dn.random_params(net, seed=4)
    for b, p in list(zip(net.param_layers(), ps))[:8]:
        s = np.float32(np.sqrt(2.0 / b.in_size))
        assert np.abs(p.weights).max() <= s and np.abs(p.weights).max() > 0.5 * s
        assert not p.biases.any() and (p.scales == 1).all()
        assert not p.rolling_mean.any() and not p.rolling_var.any()


# ---- the restatement against a textbook LSTM ----------------------------------------------

def test_oracle_forward_against_a_float64_lstm(ora):
    """Forward only, zero initial state, no batch norm: within 1e-4, the
    project's bound for activations and GEMM (README.md)."""
    S, T, I, O = 3, 4, 7, 5
    net = plan(f"[net]\nbatch={S}\ntime_steps={T}\ninputs={I}\n[lstm]\noutput={O}\n")
    params = dn.random_params(net, seed=12)
    rng = np.random.default_rng(12)
    for p in params:
        p.biases[:] = rng.uniform(-0.5, 0.5, p.biases.size)
    x = rng.uniform(-1, 1, (T, S, I)).astype(np.float32)
    ref = LstmRefNet(ora, net, params)
    ref.forward(x, training=False)
    W = {g: (p.weights.astype(np.float64), p.biases.astype(np.float64))
         for g, p in zip(dn.LSTM_GATES, params)}
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))  # noqa: E731
    c, h = np.zeros((S, O)), np.zeros((S, O))
    for t in range(T):
        a = {g: h @ W["w" + g][0].T + W["w" + g][1] + x[t].astype(np.float64) @ W["u" + g][0].T
             + W["u" + g][1] for g in "figo"}
        c = sig(a["f"]) * c + sig(a["i"]) * np.tanh(a["g"])
        h = sig(a["o"]) * np.tanh(c)
        assert np.abs(ref.lstm[0]["cell"].reshape(T, S, O)[t] - c).max() < 1e-4
        assert np.abs(ref.out[0].reshape(T, S, O)[t] - h).max() < 1e-4
    assert np.abs(h).max() > 0.01
    assert np.array_equal(ref.lstm[0]["h"], ref.out[0][-S * O:])


def test_oracle_refuses_non_finite_state(ora):
    net = plan("[net]\nbatch=1\ninputs=3\n[lstm]\noutput=2\n")
    params = dn.random_params(net, seed=1)
    params[0].biases[0] = np.inf
    with pytest.raises(FloatingPointError):
        LstmRefNet(ora, net, params).forward(np.ones((1, 3), np.float32), training=False)


# ---- declarations --------------------------------------------------------------------------

def test_pascal_methods_and_exported_symbols(hiplib):
    src = (ROOT / "pascal" / "nnHip.pas").read_text()
    cls = src[src.index("TNNHip<T> = class"):src.index("property ctx")]
    for m in ("lstmGatesForward", "lstmGatesBackward"):
        assert re.search(rf"procedure\s+{m}\(", cls), m
        assert re.search(rf"procedure TNNHip<T>\.{m}\(", src), m
    for sym, nargs in (("tns_hip_lstm_gates_forward", 14), ("tns_hip_lstm_gates_backward", 22)):
        assert getattr(hiplib, sym).argtypes is not None
        assert len(getattr(hiplib, sym).argtypes) == nargs
        assert re.search(rf"function {sym}\(", src)
    hdr = (ROOT / "include" / "tns.h").read_text()
    assert "tns_hip_lstm_gates_forward(" in hdr and "tns_hip_lstm_gates_backward(" in hdr
    from tensorium_amd.nnhip import TNNHip
    assert callable(TNNHip.lstmGatesForward) and callable(TNNHip.lstmGatesBackward)


def test_seen_header_is_unchanged(tmp_path):
    net = plan("[net]\nbatch=1\ninputs=3\n[lstm]\noutput=2\n")
    path = tmp_path / "w"
    dn.write_weights(path, net, dn.random_params(net), major=0, minor=1, seen=5)
    assert struct.unpack_from("<3iI", path.read_bytes()) == (0, 1, 0, 5)
