"""A tiny char-RNN network through HipDarknetTrain / HipDarknet, bit for bit
against tests/_rnn_oracle.py: inputs 7, two stacked [rnn] (hidden 5 -> output
6, hidden 6 -> output 5), [connected] output=7, [softmax]; streams in {1, 3},
time_steps in {1, 2, 4}, batch norm off and on, activation leaky, and one case
each of activation=tanh with logistic=1 (the self sub-layer LOGISTIC) and of
``shortcut=True``.  The first rnn is layer 0 (nothing below it takes a delta),
the second lies below a connected layer and above an rnn.

Two training iterations (forward with truth, backward, update) and a third
forward, compared after every pass: every layer's output and delta in full,
``state`` in full, all three sub-layers' weights, biases, scales, update
buffers, statistics and BN inputs, and cost().  The input and self sub-layers'
deltas are compared in slice 0 only: every sub-layer backward clamps its whole
delta, so under batch norm a slice that normalizeDelta pushed outside [-1, 1]
is clamped again by a later step; nothing reads those slices afterwards, and
the fused path leaves them as the step that owned them did.  Slice 0 is
written last.  The output sub-layer's delta is the layer's own and is compared
in full.  The same comparison runs for ``rnn_fused=True`` (the fused step
kernels, the hoisted products) and ``rnn_fused=False`` (the reference's call
sequence).  With streams 3 a hidden slice is 15 and 18 floats (the scalar path
of the step kernels; later slices start off a 16-byte boundary);
``test_vector_path_inside_a_network`` has slices of 8 and 16 floats.

One stream under batch norm: the reference's unbiased variance of a single row
is 0/0, so that case compares which values are non-finite and the bits of all
others, as the lstm test does.

Inference (HipDarknet): with time_steps = 1 the state carries from call to
call and reset_state() repeats the first result; with time_steps = 3 the steps
of one call do not chain, call after call equal to the oracle."""
import numpy as np
import pytest

from tensorium_amd import darknet as dn

from _rnn_oracle import RnnRefNet

pytestmark = pytest.mark.gpu

LR, MOM, DECAY = 1e-2, 0.9, 1e-4
I = 7


def cfg(streams, steps, bn, dims=((5, 6), (6, 5)), act="leaky", logistic=0):
    body = "".join(f"[rnn]\nhidden={h}\noutput={o}\nactivation={act}\nlogistic={logistic}\n"
                   f"batch_normalize={int(bn)}\n" for h, o in dims)
    return (f"[net]\nbatch={streams}\ntime_steps={steps}\ninputs={I}\n" + body +
            f"[connected]\noutput={I}\nactivation=linear\n[softmax]\n")


def make(streams, steps, bn, seed, shortcut=False, **kw):
    net = dn.Network(dn.parse_cfg(cfg(streams, steps, bn, **kw)), rnn=True)
    for l in net.rnns():
        l.shortcut = shortcut
    params = dn.random_params(net, seed=seed)
    rng = np.random.default_rng(seed)
    for p in params:   # (drawn 0 / 1: make them take part)
        p.biases[:] = rng.uniform(-0.3, 0.3, p.biases.size)
        if p.scales is not None:
            p.scales[:] = rng.uniform(0.5, 1.5, p.scales.size)
            p.rolling_mean[:] = rng.uniform(-0.1, 0.1, p.scales.size)
            p.rolling_var[:] = rng.uniform(0.5, 2.0, p.scales.size)
    B = net.batch
    xs = [rng.uniform(-1, 1, (B, I)).astype(np.float32) for _ in range(3)]
    truths = []
    for _ in range(3):
        t = np.zeros((B, I), np.float32)
        t[np.arange(B), rng.integers(0, I, B)] = 1
        truths.append(t)
    return net, params, xs, truths


def device_state(model):
    s = {}
    for l in model.net.layers:
        i = l.index
        s[f"{i}.out"] = model.out[i]
        if hasattr(model, "delta"):
            s[f"{i}.delta"] = model.delta[i]
        if l.kind == "rnn":
            L = model.rnn[i]
            s[f"{i}.state"] = L["state"]
            for g, st in L["sub"].items():
                for k, v in st.items():
                    if k == "delta":
                        s[f"{i}.{g}.delta0"] = v[:L["S"] * st["O"]]
                    elif k not in ("I", "O", "act"):
                        s[f"{i}.{g}.{k}"] = v
        elif hasattr(model, "fc") and i in model.fc:
            for k, v in model.fc[i].items():
                s[f"{i}.{k}"] = v
    return {k: v.detach().cpu().numpy().ravel().copy() for k, v in s.items()}


def mismatches(model, want, cost, nonfinite_ok):
    got = device_state(model)
    bad = []
    for k, w in want.items():
        g = got[k]
        if nonfinite_ok:
            fin = np.isfinite(w)
            ok = np.array_equal(fin, np.isfinite(g)) and np.array_equal(
                g[fin].view(np.uint32), w[fin].view(np.uint32))
        else:
            ok = np.array_equal(g.view(np.uint32), w.view(np.uint32))
        if not ok:
            bad.append((k, int((g.view(np.uint32) != w.view(np.uint32)).sum())))
    c = np.float32(model.cost())
    if not (c == np.float32(cost) or (nonfinite_ok and not np.isfinite(c)
                                      and not np.isfinite(cost))):
        bad.append(("cost", float(c), cost))
    return bad


def reference(ora, net, params, xs, truths, nonfinite_ok):
    """The oracle's state after every pass of the sequence (computed once)."""
    ref = RnnRefNet(ora, net, params, nonfinite_ok=nonfinite_ok)
    snaps = []
    for s in range(2):
        ref.forward(xs[s], truths[s])
        snaps.append((f"forward {s}", ref.state(), ref.cost()))
        ref.backward(xs[s])
        snaps.append((f"backward {s}", ref.state(), ref.cost()))
        ref.update(LR, MOM, DECAY)
        snaps.append((f"update {s}", ref.state(), ref.cost()))
    ref.forward(xs[2], truths[2])
    snaps.append(("forward 2", ref.state(), ref.cost()))
    return snaps


def run(hip, T, net, params, xs, truths, snaps, fused, nonfinite_ok):
    model = dn.HipDarknetTrain(hip, net, params, T, rnn_fused=fused)
    X = [T.from_numpy(x).cuda() for x in xs]
    Tr = [T.from_numpy(t).cuda() for t in truths]
    it = iter(snaps)
    bad = []

    def check():
        hip.finish()
        name, want, cost = next(it)
        bad.extend((name,) + b for b in mismatches(model, want, cost, nonfinite_ok))

    for s in range(2):
        model.forward(X[s], Tr[s])
        check()
        model.backward(X[s])
        check()
        model.update(LR, MOM, DECAY)
        check()
    model.forward(X[2], Tr[2])
    check()
    for x, h in zip(X, xs):
        assert np.array_equal(x.cpu().numpy(), h), "the network input was written"
    return model, bad


def both(hip, T, ora, net, params, xs, truths, nonfinite_ok=False):
    snaps = reference(ora, net, params, xs, truths, nonfinite_ok)
    if not nonfinite_ok:
        last = snaps[-1][1]
        assert snaps[-1][2] > 0 and np.abs(last["0.self.w"]).max() > 0
        back = snaps[4][1]
        assert all(np.abs(back[k]).max() > 0 for k in
                   ("0.input.wu", "0.output.wu", "1.input.wu", "1.output.bu", "0.delta",
                    "0.input.delta0"))
        if net.time_steps > 1:
            assert np.abs(back["0.self.wu"]).max() > 0 and np.abs(back["1.self.wu"]).max() > 0
    for fused in (True, False):
        model, bad = run(hip, T, net, params, xs, truths, snaps, fused, nonfinite_ok)
        assert not bad, (f"rnn_fused={fused}", bad[:12])
    return model, snaps


@pytest.mark.parametrize("bn", [0, 1])
@pytest.mark.parametrize("steps", [1, 2, 4])
@pytest.mark.parametrize("streams", [1, 3])
def test_two_training_iterations_and_a_forward(hip, torch_cuda, ora, streams, steps, bn):
    nonfinite_ok = bool(bn) and streams == 1     # the variance of one row is 0/0
    net, params, xs, truths = make(streams, steps, bn, 300 + 10 * steps + streams)
    both(hip, torch_cuda, ora, net, params, xs, truths, nonfinite_ok)


@pytest.mark.parametrize("bn", [0, 1])
def test_tanh_with_a_logistic_self_sublayer(hip, torch_cuda, ora, bn):
    net, params, xs, truths = make(3, 4, bn, 61, act="tanh", logistic=1)
    assert net.layers[0].self_activation == dn.ACT["LOGISTIC"]
    both(hip, torch_cuda, ora, net, params, xs, truths)


@pytest.mark.parametrize("bn", [0, 1])
def test_shortcut(hip, torch_cuda, ora, bn):
    net, params, xs, truths = make(3, 4, bn, 62, shortcut=True)
    _, snaps = both(hip, torch_cuda, ora, net, params, xs, truths)
    plain = reference(ora, *make(3, 4, bn, 62), False)
    assert not np.array_equal(snaps[0][1]["0.state"], plain[0][1]["0.state"])


def test_the_later_clamps_of_the_layers_delta_matter(ora):
    """(no GPU work) under batch norm the whole-delta clamp of a later step
    does change an earlier-processed slice of the layer's delta in this
    sequence — what the fused path has to, and is seen above to, reproduce:
    after a backward every element of slices 1 .. T-1 lies in [-1, 1], and
    some sit on the bound."""
    net, params, xs, truths = make(3, 4, 1, 62, shortcut=True)
    snaps = reference(ora, net, params, xs, truths, False)
    hit = 0
    for name, s, _ in snaps:
        if name.startswith("backward"):
            for i, l in enumerate(net.rnns()):
                d = s[f"{i}.delta"][3 * l.filters:]
                assert np.abs(d).max() <= 1.0
                hit += int((np.abs(d) == 1.0).sum())
    assert hit > 0


def test_vector_path_inside_a_network(hip, torch_cuda, ora):
    """streams * hidden a multiple of 4 (8 and 16 floats a step): every slice
    16-byte aligned, the step kernels' float4 path."""
    net, params, xs, truths = make(2, 3, 1, 77, dims=((4, 8), (8, 4)))
    model, _ = both(hip, torch_cuda, ora, net, params, xs, truths)
    L = model.rnn[0]
    assert L["n"] % 4 == 0 and L["state"].data_ptr() % 16 == 0
    net, params, xs, truths = make(2, 3, 0, 78, dims=((4, 8), (8, 4)))
    both(hip, torch_cuda, ora, net, params, xs, truths)


def test_an_lstm_and_an_rnn_in_one_network(hip, torch_cuda):
    """Both kinds' blocks carry a ``gate``: each goes to the mixin of the layer
    that owns it.  (No oracle covers the mix; the fused and the literal paths
    of both layers agree bit for bit and the rnn sits on the lstm's output.)"""
    T = torch_cuda
    net = dn.Network(dn.parse_cfg(
        f"[net]\nbatch=3\ntime_steps=2\ninputs={I}\n[lstm]\noutput=5\n"
        f"[rnn]\nhidden=4\noutput=6\nactivation=leaky\n"
        f"[connected]\noutput={I}\nactivation=linear\n[softmax]\n"), rnn=True)
    params = dn.random_params(net, seed=5)
    rng = np.random.default_rng(5)
    x = T.from_numpy(rng.uniform(-1, 1, (net.batch, I)).astype(np.float32)).cuda()
    t = np.zeros((net.batch, I), np.float32)
    t[np.arange(net.batch), rng.integers(0, I, net.batch)] = 1
    truth = T.from_numpy(t).cuda()
    states = []
    for fused in (True, False):
        m = dn.HipDarknetTrain(hip, net, params, T, lstm_fused=fused, rnn_fused=fused)
        assert sorted(m.lstm) == [0] and sorted(m.rnn) == [1]
        assert sorted(m.lstm[0]["sub"]) == sorted(dn.LSTM_GATES)
        assert list(m.rnn[1]["sub"]) == list(dn.RNN_SUBS)
        for _ in range(2):
            m.forward(x, truth)
            m.backward(x)
            m.update(LR, MOM, DECAY)
        hip.finish()
        s = device_state(m)
        s.update({f"0.{g}.w": st["w"].cpu().numpy().ravel() for g, st in m.lstm[0]["sub"].items()})
        assert all(np.isfinite(v).all() for v in s.values())
        assert s["0.wf.w"].any() and np.abs(s["0.delta"]).max() > 0    # the rnn passed a delta down
        states.append(s)
    for k, v in states[0].items():
        assert np.array_equal(v.view(np.uint32), states[1][k].view(np.uint32)), k


# ---- inference ---------------------------------------------------------------------------

def infer_equal(hip, T, ora, net, params, xs, fused, calls):
    ref = RnnRefNet(ora, net, params)
    model = dn.HipDarknet(hip, net, params, T, rnn_fused=fused)
    results = []
    for c in range(calls):
        x = xs[c % len(xs)]
        ref.forward(x, training=False)
        X = T.from_numpy(x).cuda()
        outs = [o.cpu().numpy().copy() for o in model.forward(X)]
        for i, o in enumerate(outs):
            assert np.array_equal(o.view(np.uint32), ref.out[i].view(np.uint32)), (c, i)
        for i, L in model.rnn.items():
            assert np.array_equal(L["state"].cpu().numpy().view(np.uint32),
                                  ref.rnn[i]["state"].view(np.uint32)), (c, i, "state")
        assert np.array_equal(X.cpu().numpy(), x), "the network input was written"
        results.append(outs)
    return model, results


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("bn", [0, 1])
def test_inference_time_steps_1_carries_the_state(hip, torch_cuda, ora, fused, bn):
    net, params, xs, _ = make(2, 1, bn, 41)
    x = [xs[0]]                                       # the same input, call after call
    model, res = infer_equal(hip, torch_cuda, ora, net, params, x, fused, 4)
    for a, b in zip(res, res[1:]):                    # the state goes on: another result
        assert not np.array_equal(a[0], b[0])
    model.reset_state()
    again = [o.cpu().numpy().copy() for o in model.forward(torch_cuda.from_numpy(x[0]).cuda())]
    for i, (a, b) in enumerate(zip(again, res[0])):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), ("reset", i)
    assert np.allclose(res[0][-1].reshape(-1, I).sum(1), 1, atol=1e-5)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("shortcut", [False, True])
def test_inference_steps_of_one_call_do_not_chain(hip, torch_cuda, ora, fused, shortcut):
    net, params, xs, _ = make(2, 3, 1, 42, shortcut=shortcut)
    model, res = infer_equal(hip, torch_cuda, ora, net, params, [xs[0]], fused, 3)
    O = net.batch // 3 * net.layers[0].filters        # one step's slice of layer 0's output
    assert not np.array_equal(res[0][0][O:2 * O], res[1][0][O:2 * O])   # step 1: call to call
    # the first call's step 1 read state[1] as constructed: the self sub-layer saw zeros,
    # whatever step 0 had just written
    assert not model.rnn[0]["state"][3 * model.rnn[0]["n"]:].any()
