"""The rnn layer without a GPU: the planner (``[rnn]`` as parseRNN reads it),
the .weights layout of its three connected blocks, ``rnn_cfg``, the routing of
a layer's blocks by its kind, and the properties of the CPU restatement
tests/_rnn_oracle.py that the reference's loops imply: what a training and an
inference forward carry, and the signed zero of the forward's two adds against
the backward's one."""
import numpy as np
import pytest

from tensorium_amd import darknet as dn

from _rnn_oracle import RnnRefNet, state_forward

ACT = dn.ACT


def plan(cfg, batch=None):
    return dn.Network(dn.parse_cfg(cfg), batch, rnn=True)


def tiny(streams, steps, bn=0, act="leaky", extra="", inputs=7, hidden=5, output=6):
    return (f"[net]\nbatch={streams}\ntime_steps={steps}\ninputs={inputs}\n"
            f"[rnn]\noutput={output}\nhidden={hidden}\nactivation={act}\n"
            f"batch_normalize={int(bn)}\n{extra}"
            f"[connected]\noutput={inputs}\nactivation=linear\n[softmax]\n")


# ---- planner -------------------------------------------------------------------------

def test_rnn_options_and_defaults():
    net = plan("[net]\nbatch=2\ntime_steps=3\ninputs=9\n[rnn]\n"
               "[rnn]\noutput=4\nhidden=5\nactivation=tanh\nlogistic=1\nbatch_normalize=1\n")
    a, b = net.layers
    assert net.batch == 6
    assert (a.kind, a.filters, a.hidden, a.bn, a.in_size, a.steps) == ("rnn", 1, 1, False, 9, 3)
    assert a.activation == a.self_activation == ACT["LOGISTIC"]      # parseRNN's default
    assert (a.out_c, a.out_h, a.out_w, a.shortcut) == (1, 1, 1, False)
    assert (b.filters, b.hidden, b.bn, b.in_size, b.out_size) == (4, 5, True, 1, 4)
    assert (b.activation, b.self_activation) == (ACT["TANH"], ACT["LOGISTIC"])
    assert [l.index for l in net.rnns()] == [0, 1] and net.lstms() == []
    b.shortcut = True                                   # a public field, no cfg key
    assert net.layers[1].shortcut
    # logistic=0: the self sub-layer takes the layer's activation
    c = plan(tiny(2, 1, act="relu")).layers[0]
    assert c.activation == c.self_activation == ACT["RELU"]


def test_the_default_plan_still_refuses_rnn_and_names_the_argument():
    """``Network(sections, batch)`` keeps refusing ``[rnn]`` as it did before
    the layer was built (tests/test_lstm.py holds it to that); ``rnn=True``
    plans it."""
    cfg = tiny(2, 3)
    with pytest.raises(ValueError, match=r"\[rnn\] layer is not yet implemented.*rnn=True"):
        dn.Network(dn.parse_cfg(cfg))
    with pytest.raises(ValueError, match="rnn=True"):
        dn.Network(dn.parse_cfg(dn.rnn_cfg(2, 3)), None, False)
    assert dn.Network(dn.parse_cfg(cfg), rnn=True).layers[0].kind == "rnn"
    # the argument changes nothing else: an lstm plan is the same either way
    a = dn.Network(dn.parse_cfg(dn.lstm_cfg(2, 3, inputs=7, hidden=5, layers=1)))
    b = dn.Network(dn.parse_cfg(dn.lstm_cfg(2, 3, inputs=7, hidden=5, layers=1)), rnn=True)
    assert a.layers == b.layers and a.batch == b.batch


def test_rnn_sets_flat_like_lstm():
    with pytest.raises(ValueError, match="refused"):
        plan("[net]\nbatch=2\nwidth=4\nheight=4\nchannels=1\n[rnn]\noutput=16\n"
             "[maxpool]\nsize=2\nstride=2\n")
    assert plan("[net]\nbatch=2\nwidth=4\nheight=4\nchannels=2\n[rnn]\noutput=3\n"
                ).layers[0].in_size == 32


@pytest.mark.parametrize("body, what", [
    ("[rnn]\noutput=0\n", "layer 0"),
    ("[rnn]\noutput=3\nhidden=0\n", "layer 0"),
    ("[rnn]\noutput=3\nlogistic=2\n", "LOGGY"),
    ("[rnn]\noutput=3\nactivation=elu\n", "layer 0.*elu"),
    ("[rnn]\noutput=3\nactivation=loggy\n", "layer 0.*loggy"),
    ("[connected]\noutput=4\n[rnn]\noutput=3\nactivation=selu\n", "layer 1"),
])
def test_refusals(body, what):
    with pytest.raises(ValueError, match=what):
        plan("[net]\nbatch=2\ninputs=9\n" + body)


def test_refusals_of_shape():
    with pytest.raises(ValueError, match="inputs"):
        plan("[net]\nbatch=2\n[rnn]\noutput=4\n")
    cfg = tiny(5, 4)
    assert plan(cfg).batch == 20
    with pytest.raises(ValueError, match=r"\[rnn\] layer 0.*time_steps"):
        plan(cfg, batch=10)                         # the reference truncates 10 div 4


def test_rnn_cfg_parses_and_plans():
    net = plan(dn.rnn_cfg(batch=32, time_steps=16))
    assert (net.batch, net.time_steps, net.inputs) == (512, 16, 256)
    assert [l.kind for l in net.layers] == ["rnn"] * 3 + ["connected", "softmax", "cost"]
    for l, i in zip(net.layers[:3], (256, 1024, 1024)):
        assert (l.in_size, l.filters, l.hidden, l.bn, l.steps, l.activation,
                l.self_activation) == (i, 1024, 1024, True, 16, ACT["LEAKY"], ACT["LEAKY"])
    fc = net.layers[3]
    assert (fc.in_size, fc.filters, fc.activation) == (1024, 256, ACT["LINEAR"])
    small = plan(dn.rnn_cfg(3, 2, inputs=7, hidden=5, layers=1, bn=False, activation="tanh",
                            cost=False))
    assert [l.kind for l in small.layers] == ["rnn", "connected", "softmax"]
    assert not small.layers[0].bn and small.batch == 6
    assert small.layers[0].activation == ACT["TANH"]
    assert "not a file" in dn.rnn_cfg.__doc__


# ---- weights --------------------------------------------------------------------------

@pytest.mark.parametrize("bn", [False, True])
def test_three_blocks_in_file_order_and_weights_round_trip(tmp_path, bn):
    I, H, O = 7, 5, 6
    cfg = (f"[net]\nbatch=2\ntime_steps=3\ninputs={I}\n"
           f"[rnn]\noutput={O}\nhidden={H}\nactivation=tanh\nlogistic=1\n"
           f"batch_normalize={int(bn)}\n"
           f"[rnn]\noutput={H}\nhidden={O}\nactivation=leaky\nbatch_normalize={int(bn)}\n"
           f"[connected]\noutput={I}\nactivation=linear\n")
    net = plan(cfg)
    blocks = net.param_layers()
    assert [b.gate for b in blocks] == list(dn.RNN_SUBS) * 2 + [""]
    assert [b.index for b in blocks] == [0] * 3 + [1] * 3 + [2]
    assert [(b.filters, b.in_size) for b in blocks] == [(H, I), (H, H), (O, H), (O, O), (O, O),
                                                        (H, O), (I, H)]
    assert [b.activation for b in blocks[:3]] == [ACT["TANH"], ACT["LOGISTIC"], ACT["TANH"]]
    assert all(b.kind == "connected" and b.bn == bn for b in blocks[:6])
    params = dn.random_params(net, seed=9)
    rng = np.random.default_rng(1)
    for p in params:   # (biases are drawn 0, scales 1: make every array distinct)
        p.biases[:] = rng.uniform(-1, 1, p.biases.size)
        if p.scales is not None:
            for a in (p.scales, p.rolling_mean, p.rolling_var):
                a[:] = rng.uniform(0.5, 1.5, a.size)
    path = tmp_path / "rnn.weights"
    dn.write_weights(path, net, params, seen=77)
    data = path.read_bytes()
    off = 20                                        # 3 int32 + uint64 seen
    for b, p in zip(blocks, params):                # loadConnectedWeights' layout, block by block
        assert p.weights.shape == (b.filters, b.in_size)
        parts = [p.biases, p.weights.ravel()] + ([p.scales, p.rolling_mean, p.rolling_var]
                                                 if b.bn else [])
        for a in parts:
            assert np.array_equal(np.frombuffer(data, "<f4", a.size, off), a), (b.index, b.gate)
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


def test_blocks_are_routed_by_the_owning_layers_kind():
    """An lstm and an rnn layer in one network: each driver hands a block to
    the mixin of the layer that owns it (both carry a non-empty ``gate``)."""
    net = plan("[net]\nbatch=2\ntime_steps=2\ninputs=5\n[lstm]\noutput=3\n[rnn]\noutput=4\n"
               "hidden=2\n[connected]\noutput=5\n")
    blocks = net.param_layers()
    kinds = [net.layers[b.index].kind if b.gate else "" for b in blocks]
    assert kinds == ["lstm"] * 8 + ["rnn"] * 3 + [""]


# ---- the oracle's loops --------------------------------------------------------------

def make(cfg, seed, shortcut=False):
    net = plan(cfg)
    for l in net.rnns():
        l.shortcut = shortcut
    params = dn.random_params(net, seed=seed)
    rng = np.random.default_rng(seed)
    for p in params:
        p.biases[:] = rng.uniform(-0.3, 0.3, p.biases.size)
    x = rng.uniform(-1, 1, (net.batch, net.inputs)).astype(np.float32)
    t = np.zeros((net.batch, net.inputs), np.float32)
    t[np.arange(net.batch), rng.integers(0, net.inputs, net.batch)] = 1
    return net, params, x, t


@pytest.mark.parametrize("shortcut", [False, True])
def test_training_zeroes_state0_and_carries_nothing(ora, shortcut):
    net, params, x, t = make(tiny(3, 4), 11, shortcut)
    ref = RnnRefNet(ora, net, params)
    n = ref.rnn[0]["n"]
    ref.forward(x, t)
    first = ref.state()
    assert not first["0.state"][:n].any() and first["0.state"][n:].all()
    ref.forward(x, t)                                # nothing was updated in between
    again = ref.state()
    for k in ("0.state", "0.out", "1.out", "2.out", "0.input.out", "0.self.out"):
        assert np.array_equal(first[k].view(np.uint32), again[k].view(np.uint32)), k
    ref.backward(x)
    assert ref.state()["0.input.wu"].any() and ref.state()["0.self.wu"].any()
    if shortcut:   # the backward's recompute drops the state[i] term the forward carried
        assert not np.array_equal(ref.state()["0.state"][2 * n:], first["0.state"][2 * n:])


def test_inference_steps_of_one_call_do_not_chain(ora):
    net, params, x, _ = make(tiny(1, 3), 12)
    ref = RnnRefNet(ora, net, params)
    ref.forward(x, training=False)
    one = [o.copy() for o in ref.out]
    n = ref.rnn[0]["n"]
    assert ref.rnn[0]["state"][:3 * n].any() and not ref.rnn[0]["state"][3 * n:].any()
    ref.forward(x, training=False)                   # the same input again
    two = [o.copy() for o in ref.out]
    O = net.layers[0].out_size
    assert not np.array_equal(one[0][O:2 * O], two[0][O:2 * O])      # step 1 differs
    # ... because it read what the first call's step 1 left, not this call's step 0:
    fresh = RnnRefNet(ora, net, params)
    fresh.rnn[0]["state"][:] = 0
    fresh.forward(x, training=False)
    assert np.array_equal(fresh.out[0], one[0])
    ref.reset_state()
    ref.forward(x, training=False)
    assert np.array_equal(ref.out[0].view(np.uint32), one[0].view(np.uint32))


def test_inference_time_steps_1_chains_call_to_call(ora):
    net, params, x, _ = make(tiny(2, 1), 13)
    ref = RnnRefNet(ora, net, params)
    L = ref.rnn[0]
    outs = []
    for _ in range(3):
        before = L["state"][:L["n"]].copy()
        ref.forward(x, training=False)
        outs.append(ref.out[0].copy())
        # state[0] = 0 + act(W x + b) + act(U state[0] + b'): the second term saw `before`
        si, ss = L["sub"]["input"], L["sub"]["self"]
        assert np.array_equal(L["state"][:L["n"]],
                              (np.float32(0) + si["out"][:L["n"]]) + ss["out"][:L["n"]])
        assert not np.array_equal(before, L["state"][:L["n"]])
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    assert not L["state"][L["n"]:].any()             # state[1] is training's


def test_signed_zero_forward_two_adds_backward_one(ora):
    """a = b = -0: the forward's fill, add, add gives (0 + -0) + -0 = +0, the
    backward's single add -0 + -0 = -0."""
    nz = np.full(3, -0.0, np.float32)
    a, b, s = state_forward(ora, nz, None, ACT["LINEAR"], nz, None, ACT["LINEAR"], None, 3)
    assert np.signbit(a).all() and np.signbit(b).all() and not np.signbit(s).any()
    a, b, s = state_forward(ora, nz, None, ACT["LINEAR"], nz, None, ACT["LINEAR"], nz, 3)
    assert np.signbit(s).all()                       # the shortcut's copy keeps the sign
    # the backward's recompute, through the layer: the two sub-layers' outputs at -0
    net, params, x, t = make(tiny(2, 2, act="linear"), 14)
    ref = RnnRefNet(ora, net, params)
    ref.forward(x, t)
    L = ref.rnn[0]
    n = L["n"]
    L["sub"]["input"]["out"][:] = -0.0
    L["sub"]["self"]["out"][:] = -0.0
    ref.backward(x)
    assert np.signbit(L["state"][n:]).all() and not L["state"][n:].any()
