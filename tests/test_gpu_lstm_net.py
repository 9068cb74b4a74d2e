"""A tiny char-LSTM network through HipDarknetTrain / HipDarknet, bit for bit
against tests/_lstm_oracle.py: inputs 7, two stacked [lstm] (outputs 5 and 6),
[connected] output=7, [softmax]; streams in {1, 3}, time_steps in {1, 2, 4},
batch norm off and on.

Two training iterations (forward with truth, backward, update) and a third
forward — the carry of c, h and dc, the stale step-0 operands, the rolling
statistics and momentum — compared after every pass: every layer's output and
delta, cell, the five state buffers, all sub-layers' weights, biases, scales,
their update buffers, statistics and BN inputs, and cost().  A sub-layer's
delta is scratch outside the slice written last.  The same comparison runs
for ``lstm_fused=True`` (the fused gate kernels, the hoisted and batched
GEMMs) and ``lstm_fused=False`` (the reference's call sequence).  With streams
3 a step's slice is 15 and 18 floats (the scalar path of the gate kernels; the
second layer's slices start off a 16-byte boundary), with streams 1 and
outputs 5 / 6 likewise; ``test_vector_path_inside_a_network`` has slices of 8
and 16 floats.

One stream under batch norm: the reference's unbiased variance of a single row
is 0/0, so its rolling variance and, from the first backward on, its
parameters are NaN.  There the oracle's finiteness assertion cannot hold by the
reference's own arithmetic; that case compares which values are non-finite and
the bits of all others.

Inference: T single-step forwards at batch 1, time_steps 1 equal one forward
at time_steps T (state carried between calls), and after reset_state() the
first result repeats."""
import numpy as np
import pytest

from tensorium_amd import darknet as dn

from _lstm_oracle import LstmRefNet

pytestmark = pytest.mark.gpu

LR, MOM, DECAY = 1e-2, 0.9, 1e-4
I = 7


def cfg(streams, steps, bn, outs=(5, 6)):
    body = "".join(f"[lstm]\noutput={o}\nbatch_normalize={int(bn)}\n" for o in outs)
    return (f"[net]\nbatch={streams}\ntime_steps={steps}\ninputs={I}\n" + body +
            f"[connected]\noutput={I}\nactivation=linear\n[softmax]\n")


def make(streams, steps, bn, seed, outs=(5, 6)):
    net = dn.Network(dn.parse_cfg(cfg(streams, steps, bn, outs)))
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
        if l.kind == "lstm":
            L = model.lstm[i]
            for k in ("c", "h", "dc", "prevCell", "prevState", "cell"):
                s[f"{i}.{k}"] = L[k]
            for g, st in L["sub"].items():
                for k, v in st.items():
                    if k == "delta":
                        s[f"{i}.{g}.delta0"] = v[:L["n"]]
                    elif k != "I":
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
    ref = LstmRefNet(ora, net, params, nonfinite_ok=nonfinite_ok)
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
    model = dn.HipDarknetTrain(hip, net, params, T, lstm_fused=fused)
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


@pytest.mark.parametrize("bn", [0, 1])
@pytest.mark.parametrize("steps", [1, 2, 4])
@pytest.mark.parametrize("streams", [1, 3])
def test_two_training_iterations_and_a_forward(hip, torch_cuda, ora, streams, steps, bn):
    nonfinite_ok = bool(bn) and streams == 1     # the variance of one row is 0/0
    net, params, xs, truths = make(streams, steps, bn, 300 + 10 * steps + streams)
    snaps = reference(ora, net, params, xs, truths, nonfinite_ok)
    last = snaps[-1][1]
    if not nonfinite_ok:
        assert snaps[-1][2] > 0 and np.abs(last["0.wf.w"]).max() > 0
        assert np.abs(snaps[4][1]["0.dc"]).max() > 0
    for fused in (True, False):
        model, bad = run(hip, torch_cuda, net, params, xs, truths, snaps, fused, nonfinite_ok)
        assert not bad, (f"lstm_fused={fused}", bad[:12])


def test_vector_path_inside_a_network(hip, torch_cuda, ora):
    """streams * outputs a multiple of 4 (8 and 16 floats a step): every slice
    16-byte aligned, the gate kernels' float4 path."""
    net, params, xs, truths = make(2, 3, 1, 77, outs=(4, 8))
    snaps = reference(ora, net, params, xs, truths, False)
    for fused in (True, False):
        model, bad = run(hip, torch_cuda, net, params, xs, truths, snaps, fused, False)
        assert not bad, (f"lstm_fused={fused}", bad[:12])
    L = model.lstm[0]
    assert L["n"] % 4 == 0 and L["cell"].data_ptr() % 16 == 0


def test_stale_step0_operands_are_zero_at_first(ora):
    """(no GPU work) steps = 1: the first backward's f-gate delta and w* dW
    products read prevCell / prevState as constructed, zeros."""
    net, params, xs, truths = make(3, 1, 0, 5)
    ref = LstmRefNet(ora, net, params)
    ref.forward(xs[0], truths[0])
    ref.backward(xs[0])
    s = ref.state()
    assert not s["0.wf.wu"].any() and not s["0.wo.wu"].any() and not s["0.wf.delta0"].any()
    assert s["0.uo.wu"].any() and s["0.wo.delta0"].any() and s["0.c"].any()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("bn", [0, 1])
def test_inference_state_carry(hip, torch_cuda, ora, fused, bn):
    T, steps = torch_cuda, 4
    net, params, xs, _ = make(1, steps, bn, 41)
    one = dn.Network(dn.parse_cfg(cfg(1, 1, bn)))
    x = xs[0]
    ref = LstmRefNet(ora, net, params)
    ref.forward(x, training=False)
    whole = dn.HipDarknet(hip, net, params, T, lstm_fused=fused)
    outs = [o.cpu().numpy().copy() for o in whole.forward(T.from_numpy(x).cuda())]
    for i, o in enumerate(outs):
        assert np.array_equal(o.view(np.uint32), ref.out[i].view(np.uint32)), ("oracle", i)
    step = dn.HipDarknet(hip, one, params, T, lstm_fused=fused)

    def stepwise():
        rows = []
        for t in range(steps):
            o = step.forward(T.from_numpy(x[t:t + 1].copy()).cuda())
            rows.append([a.cpu().numpy().copy() for a in o])
        return [np.concatenate([r[i] for r in rows]) for i in range(len(net.layers))]

    first = stepwise()
    for i, (a, b) in enumerate(zip(first, outs)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), ("carry", i)
    again = stepwise()          # the state goes on: another result
    assert not np.array_equal(again[0], first[0])
    step.reset_state()
    for i, (a, b) in enumerate(zip(stepwise(), first)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), ("reset", i)
    assert np.allclose(outs[-1].reshape(steps, I).sum(1), 1, atol=1e-5)
