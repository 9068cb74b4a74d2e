"""CPU restatement of TRNNLayer.forward / backward / update (the CPU path,
nrnnlayer.pas:148-257, 345-400), written from the Pascal loops and composed
from the oracle's restated calls (sgemm, add_bias, activate, gradient,
batch_norm, normalize, add_sums, add_dots, mean_var_delta, normalize_delta,
ora_clamp, sgd_update) the way tests/_lstm_oracle.py composes its sub-layers.
``RnnRefNet`` extends tests/_classifier_oracle.RefNet, whose connected, softmax
and cost layers it keeps.

* ``state_forward`` / ``delta_backward``: one step's elementwise stage, per
  element, each arithmetic operation one float32 rounding (numpy float32
  arrays), activations and gradients through ora.activate / ora.gradient.
* The three sub-layers input, self, output are TConnectedLayer.forward /
  backward (nconnectedlayer.pas:157-322) with their step / inputStep /
  deltaStep offsets and groups = the layer's batch (streams).  Rows are
  [step][stream].  The output sub-layer's output and delta are the layer's
  arrays.
* Reproduced, not repaired: a training forward zeroes state[0] and writes
  state[i + 1], an inference forward zeroes nothing and step i writes the
  slice state[i] it read (so the steps of one call do not chain); the forward
  sums (0 or state[i]) + a, then + b; the backward overwrites state[i + 1] by
  the one add a + b; every sub-layer backward clamps its whole delta.
* Everything a pass produces is asserted finite (``check_finite``) unless the
  caller asks otherwise (``nonfinite_ok``: batch norm over one stream, where
  the reference's unbiased variance is 0/0)."""
import numpy as np

from tensorium_amd.darknet import RNN_SUBS

import _heads_oracle as ho
from _classifier_oracle import RefNet, _c

f32 = np.float32


def _clamp1(ora, a):
    ora._lib2().ora_clamp(ora._p(a), a.size, -1.0, 1.0)
    return a


def state_forward(ora, a, a_bias, a_act, b, b_bias, b_act, prev, H):
    """The elementwise calls of rnnStepForward between the products and the
    output sub-layer: (bias, column k mod H) and activation on the two slices,
    then fill (or the copy of prev), add, add.  Returns (a, b, state)."""
    a, b = _c(a).copy(), _c(b).copy()
    col = np.arange(a.size) % H
    if a_bias is not None:
        a = a + _c(a_bias)[col]
    ora.activate(a, a_act)
    if b_bias is not None:
        b = b + _c(b_bias)[col]
    ora.activate(b, b_act)
    s = np.zeros(a.size, f32) if prev is None else _c(prev).copy()
    s = s + a
    s = s + b
    return a, b, s


def delta_backward(ora, delta, out, act, out2=None, act2=None):
    """clamp + Derivative on one slice; with out2 also the copy and the next
    sub-layer's clamp + Derivative.  Returns (delta, delta2 or None)."""
    d = ora.gradient(_c(out), act, _clamp1(ora, _c(delta).copy()))
    if out2 is None:
        return d, None
    return d, ora.gradient(_c(out2), act2, _clamp1(ora, d.copy()))


class RnnRefNet(RefNet):
    def __init__(self, ora, net, params, nonfinite_ok=False):
        super().__init__(ora, net, params)
        self.nonfinite_ok = nonfinite_ok
        self.rnn = {}
        for l in net.rnns():
            self.st.pop(l.index, None)
            T = l.steps
            S = net.batch // T
            self.rnn[l.index] = {"S": S, "T": T, "n": S * l.hidden, "m": S * l.filters,
                                 "state": np.zeros((T + 1) * S * l.hidden, f32), "sub": {}}
        for b, p in zip(net.param_layers(), params):
            if not b.gate:
                continue
            L = self.rnn[b.index]
            O, tn = b.filters, L["T"] * L["S"] * b.filters
            own = b.gate == "output"
            st = {"I": b.in_size, "O": O, "act": b.activation, "bn": b.bn,
                  "w": _c(p.weights).ravel().copy(), "b": _c(p.biases).copy(),
                  "wu": np.zeros(p.weights.size, f32), "bu": np.zeros(O, f32),
                  "out": self.out[b.index] if own else np.zeros(tn, f32),
                  "delta": self.delta[b.index] if own else np.zeros(tn, f32)}
            if b.bn:
                st.update(scales=_c(p.scales).copy(), rm=_c(p.rolling_mean).copy(),
                          rv=_c(p.rolling_var).copy(), x=np.zeros(tn, f32), xn=np.zeros(tn, f32))
                for k in ("su", "mean", "var", "md", "vd"):
                    st[k] = np.zeros(O, f32)
            L["sub"][b.gate] = st

    # -- TConnectedLayer.forward / backward on one step's slice -----------------
    def _sub_forward(self, L, st, step, inp, in_step, training):
        ora, S, O, I = self.ora, L["S"], st["O"], st["I"]
        n = S * O
        a = inp[in_step * S * I:(in_step + 1) * S * I]
        o = st["out"][step * n:(step + 1) * n]
        ora.sgemm(False, True, S, O, I, 1.0, a, I, st["w"], I, 0.0, o, O)
        if st["bn"]:
            if training:   # one mean / variance pair, overwritten every step
                m, v, x, xn = ora.batch_norm(o, S, O, 1, st["scales"], st["b"], st["rm"],
                                             st["rv"], f32(0.05), True)
                st.update(mean=m, var=v)
                st["x"][step * n:(step + 1) * n] = x
                st["xn"][step * n:(step + 1) * n] = xn
            else:
                ora.normalize(o, S, O, 1, st["rm"], st["rv"])
                ora.forward_scale(o, S, O, 1, st["scales"])
                ora.add_bias(o, st["b"], O, 1, S)
        else:
            ora.add_bias(o, st["b"], O, 1, S)
        ora.activate(o, st["act"])

    def _sub_backward(self, L, st, step, inp, in_step, sd, sd_step):
        ora, S, O, I = self.ora, L["S"], st["O"], st["I"]
        n = S * O
        sl = slice(step * n, (step + 1) * n)
        _clamp1(ora, st["delta"])          # delta.Clamp(-1, 1): the whole tensor
        d = st["delta"][sl]
        ora.gradient(st["out"][sl], st["act"], d)
        ora.add_sums(st["bu"], d, S, O, 1)
        if st["bn"]:
            x = st["x"][sl]
            ora.add_dots(st["su"], st["xn"][sl], d, S, O, 1)
            ora.forward_scale(d, S, O, 1, st["scales"])
            st["md"], st["vd"] = ora.mean_var_delta(d, x, st["mean"], st["var"], S, O, 1)
            ora.normalize_delta(x, st["mean"], st["var"], st["md"], st["vd"], d, S, O, 1)
        a = inp[in_step * S * I:(in_step + 1) * S * I]
        ora.sgemm(True, False, O, I, S, 1.0, d, O, a, I, 1.0, st["wu"], I)
        if sd is not None:
            ora.sgemm(False, False, S, I, O, 1.0, d, O, st["w"], I, 1.0,
                      sd[sd_step * S * I:(sd_step + 1) * S * I], I)

    # -- TRNNLayer.forward / backward ---------------------------------------------
    def _rnn_forward(self, l, inp, training):
        L = self.rnn[l.index]
        T, n, state = L["T"], L["n"], L["state"]
        si, ss, so = (L["sub"][g] for g in RNN_SUBS)
        if training:
            for st in (so, ss, si):
                np.multiply(st["delta"], f32(0), out=st["delta"])
            state[:n] = 0
        for i in range(T):
            sl = slice(i * n, (i + 1) * n)
            self._sub_forward(L, si, i, inp, i, training)
            self._sub_forward(L, ss, i, state, i, training)
            j = i + 1 if training else i
            sj = slice(j * n, (j + 1) * n)
            if l.shortcut:
                state[sj] = state[sl].copy()
            else:
                state[sj] = 0
            state[sj] = state[sj] + si["out"][sl]
            state[sj] = state[sj] + ss["out"][sl]
            self._sub_forward(L, so, i, state, j, training)

    def _rnn_backward(self, l, inp, sd):
        L = self.rnn[l.index]
        T, n, state = L["T"], L["n"], L["state"]
        si, ss, so = (L["sub"][g] for g in RNN_SUBS)
        for i in range(T - 1, -1, -1):
            sl = slice(i * n, (i + 1) * n)
            state[(i + 1) * n:(i + 2) * n] = si["out"][sl] + ss["out"][sl]
            self._sub_backward(L, so, i, state, i + 1, ss["delta"], i)
            self._sub_backward(L, ss, i, state, i, ss["delta"] if i else None, i - 1)
            si["delta"][sl] = ss["delta"][sl]
            if i and l.shortcut:
                pl = slice((i - 1) * n, i * n)
                ss["delta"][pl] = ss["delta"][pl] + ss["delta"][sl]
            self._sub_backward(L, si, i, inp, i, sd, i)

    # -- passes ------------------------------------------------------------------------
    def forward(self, x, truth=None, training=True):
        ora = self.ora
        prev = _c(x).ravel()
        for l in self.net.layers:
            i = l.index
            if training:
                np.multiply(self.delta[i], f32(0), out=self.delta[i])
            out = self.out[i]
            if l.kind == "rnn":
                self._rnn_forward(l, prev, training)
            elif l.kind == "connected":
                self._fc_forward(l, prev, training)
            elif l.kind == "softmax":
                out[:] = ora.softmax_rows(_c(prev), l.in_size // l.groups, l.temperature)
                if truth is not None and not l.noloss:
                    d, e = ora.softmax_xent(out, _c(truth).ravel())
                    self.delta[i][:] = d
                    self.loss[i][:] = e
                    self.costs[i] = f32(ora.vssum(self.loss[i]))
            elif l.kind == "cost":
                if truth is not None:
                    d, e = ho.cost_l2(prev, _c(truth).ravel())
                    self.delta[i][:] = d
                    out[:] = e
                    self.costs[i] = f32(ora.vssum(out))
            else:
                raise ValueError(l.kind)
            prev = out
        self.check_finite()

    def backward(self, x):
        for l in reversed(self.net.layers):
            i = l.index
            inp = _c(x).ravel() if i == 0 else self.out[i - 1]
            sd = None if i == 0 else self.delta[i - 1]
            d = self.delta[i]
            if l.kind == "rnn":
                self._rnn_backward(l, inp, sd)
            elif l.kind == "connected":
                self._fc_backward(l, inp, sd)
            elif l.kind == "softmax" and sd is not None:
                sd[:] = d + sd
            elif l.kind == "cost" and sd is not None:   # axpy: one fused multiply-add
                sd[:] = (f32(l.scale).astype(np.float64) * d.astype(np.float64)
                         + sd.astype(np.float64)).astype(f32)
        self.check_finite()

    def update(self, lr, momentum, decay):
        B = self.net.batch
        lrb = f32(f32(lr) / f32(B))
        ndb = f32(-f32(decay) * f32(B))
        for l in self.net.layers[:-1]:
            sts = ([self.rnn[l.index]["sub"][g] for g in RNN_SUBS] if l.kind == "rnn"
                   else [self.st[l.index]] if l.index in self.st else [])
            for st in sts:
                self.ora.sgd_update(st["w"], st["wu"], st["b"], st["bu"], st.get("scales"),
                                    st.get("su"), float(lrb), float(ndb), momentum)
        self.check_finite()

    def reset_state(self):
        for L in self.rnn.values():
            L["state"].fill(0)

    # -- what a comparison reads --------------------------------------------------------
    def state(self):
        """name -> array: every layer's output and delta, an rnn layer's state,
        and per (sub-)layer the parameters, update buffers, statistics and BN
        inputs.  The input and self sub-layers' deltas only in slice 0 (the
        last one written): every sub-layer backward clamps its whole delta, so
        under batch norm a slice that normalizeDelta pushed outside [-1, 1] is
        clamped again by a later step — scratch that nothing reads, which the
        fused path does not reproduce.  The output sub-layer's delta is the
        layer's and is read in full."""
        s = {}
        for l in self.net.layers:
            i = l.index
            s[f"{i}.out"], s[f"{i}.delta"] = self.out[i], self.delta[i]
            if l.kind == "rnn":
                L = self.rnn[i]
                s[f"{i}.state"] = L["state"]
                for g, st in L["sub"].items():
                    for k, v in st.items():
                        if k == "delta":
                            s[f"{i}.{g}.delta0"] = v[:L["S"] * st["O"]]
                        elif k not in ("I", "O", "act", "bn"):
                            s[f"{i}.{g}.{k}"] = v
            elif i in self.st:
                for k, v in self.st[i].items():
                    s[f"{i}.{k}"] = v
        return {k: np.array(v, f32, copy=True).ravel() for k, v in s.items()}

    def check_finite(self):
        bad = [k for k, v in self.state().items() if not np.isfinite(v).all()]
        bad += [f"cost {i}" for i, c in self.costs.items() if not np.isfinite(c)]
        if bad and not self.nonfinite_ok:
            raise FloatingPointError(f"the restated pass left non-finite values in {bad}")
        return bad
