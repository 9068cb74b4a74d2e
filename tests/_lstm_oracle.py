"""CPU restatement of TLSTMLayer.forward / backward / update
(nlstmlayer.pas:518-860), written from the Pascal loops and composed from the
oracle's restated calls (sgemm, add_bias, activate, gradient, batch_norm,
add_sums, add_dots, mean_var_delta, normalize_delta, ora_clamp, sgd_update) the
way tests/_classifier_oracle.py composes a connected layer, whose RefNet
``LstmRefNet`` extends (connected, softmax and cost layers are RefNet's).

* ``gates_forward`` / ``gates_backward``: one step's elementwise stage, per
  element, each arithmetic operation one float32 rounding (numpy float32
  arrays), activations and gradients through ora.activate / ora.gradient.
* The eight sub-layers are TConnectedLayer.forward / backward (nconnectedlayer.
  pas:157-322) with their step / inputStep / deltaStep offsets and groups =
  the layer's batch (streams).  Rows are [step][stream].
* Everything a pass produces is asserted finite (``check_finite``), so no
  comparison depends on a NaN's payload.  The one exception is the caller's to
  ask for (``nonfinite_ok``): a batch-normalized sub-layer over one stream,
  where the reference's unbiased variance is 0/0."""
import numpy as np

from tensorium_amd._abi import ACT
from tensorium_amd.darknet import LSTM_GATES

from _classifier_oracle import RefNet, _c

f32 = np.float32
LOGISTIC, TANH, LINEAR = ACT["LOGISTIC"], ACT["TANH"], ACT["LINEAR"]
STATE = ("c", "h", "dc", "prevCell", "prevState")


def _clamp1(ora, a):
    ora._lib2().ora_clamp(ora._p(a), a.size, -1.0, 1.0)
    return a


def _gates(ora, w, u):
    """f, i, g, o of one step: w / u the four pre-activation slices in the
    order f, i, g, o (addvv, then activate_array)."""
    f, i, g, o = (_c(a + b) for a, b in zip(w, u))
    ora.activate(f, LOGISTIC)
    ora.activate(i, LOGISTIC)
    ora.activate(g, TANH)
    ora.activate(o, LOGISTIC)
    return f, i, g, o


def gates_forward(ora, w, u, c):
    """nlstmlayer.pas:579-602.  Returns the new (c, h)."""
    f, i, g, o = _gates(ora, w, u)
    temp = i * g
    c = c * f
    c = c + temp
    h = ora.activate(c.copy(), TANH)
    h = h * o
    return c, h


def gates_backward(ora, w, u, cell, cprev, delta, dc):
    """nlstmlayer.pas:669-808 without the sub-layer calls.  Returns the gate
    deltas (f, i, g, o), each clamped to [-1, 1] as the sub-layer's backward
    clamps them first (nconnectedlayer.pas:261), and the new dc."""
    f, i, g, o = _gates(ora, w, u)
    temp3 = delta.copy()
    temp = ora.activate(cell.copy(), TANH)
    temp2 = temp3 * o
    ora.gradient(temp, TANH, temp2)
    temp2 = temp2 + dc
    temp = ora.activate(cell.copy(), TANH)
    temp = temp * temp3
    d_o = ora.gradient(o, LOGISTIC, temp).copy()
    d_g = ora.gradient(g, TANH, temp2 * i)
    d_i = ora.gradient(i, LOGISTIC, temp2 * g)
    d_f = ora.gradient(f, LOGISTIC, temp2 * cprev)
    new_dc = temp2 * f
    return tuple(_clamp1(ora, _c(d)) for d in (d_f, d_i, d_g, d_o)), new_dc


class LstmRefNet(RefNet):
    def __init__(self, ora, net, params, nonfinite_ok=False):
        super().__init__(ora, net, params)
        self.nonfinite_ok = nonfinite_ok
        self.lstm = {}
        for l in net.lstms():
            self.st.pop(l.index, None)
            T = l.steps
            S = net.batch // T
            n = S * l.filters
            L = {"S": S, "T": T, "n": n, "cell": np.zeros(T * n, f32), "sub": {}}
            for k in STATE:
                L[k] = np.zeros(n, f32)
            self.lstm[l.index] = L
        for b, p in zip(net.param_layers(), params):
            if not b.gate:
                continue
            L = self.lstm[b.index]
            O, tn = b.filters, L["T"] * L["n"]
            st = {"I": b.in_size, "w": _c(p.weights).ravel().copy(), "b": _c(p.biases).copy(),
                  "wu": np.zeros(p.weights.size, f32), "bu": np.zeros(O, f32),
                  "out": np.zeros(tn, f32), "delta": np.zeros(tn, f32)}
            if b.bn:
                st.update(scales=_c(p.scales).copy(), rm=_c(p.rolling_mean).copy(),
                          rv=_c(p.rolling_var).copy(), x=np.zeros(tn, f32), xn=np.zeros(tn, f32))
                for k in ("su", "mean", "var", "md", "vd"):
                    st[k] = np.zeros(O, f32)
            L["sub"][b.gate] = st

    # -- TConnectedLayer.forward / backward on one step's slice -----------------
    def _sub_forward(self, l, L, st, step, inp, in_step, training):
        ora, S, O, I, n = self.ora, L["S"], l.filters, st["I"], L["n"]
        a = inp[in_step * S * I:(in_step + 1) * S * I]
        o = st["out"][step * n:(step + 1) * n]
        ora.sgemm(False, True, S, O, I, 1.0, a, I, st["w"], I, 0.0, o, O)
        if l.bn:
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
        ora.activate(o, LINEAR)

    def _sub_backward(self, l, L, st, step, inp, in_step, sd, sd_step):
        ora, S, O, I, n = self.ora, L["S"], l.filters, st["I"], L["n"]
        sl = slice(step * n, (step + 1) * n)
        _clamp1(ora, st["delta"])          # delta.Clamp(-1, 1): the whole tensor
        d = st["delta"][sl]
        ora.gradient(st["out"][sl], LINEAR, d)
        ora.add_sums(st["bu"], d, S, O, 1)
        if l.bn:
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

    # -- TLSTMLayer.forward / backward -----------------------------------------------
    def _lstm_forward(self, l, inp, training):
        L = self.lstm[l.index]
        T, n, sub = L["T"], L["n"], L["sub"]
        if training:
            for g in LSTM_GATES:
                sub[g]["delta"].fill(0)
            self.delta[l.index].fill(0)
        for i in range(T):
            sl = slice(i * n, (i + 1) * n)
            for g in LSTM_GATES[:4]:
                self._sub_forward(l, L, sub[g], i, L["h"], 0, training)
            for g in LSTM_GATES[4:]:
                self._sub_forward(l, L, sub[g], i, inp, i, training)
            L["c"], L["h"] = gates_forward(self.ora, [sub["w" + g]["out"][sl] for g in "figo"],
                                           [sub["u" + g]["out"][sl] for g in "figo"], L["c"])
            L["cell"][sl] = L["c"]
            self.out[l.index][sl] = L["h"]

    def _lstm_backward(self, l, inp, sd):
        L = self.lstm[l.index]
        T, n, sub = L["T"], L["n"], L["sub"]
        cell, out, delta = L["cell"], self.out[l.index], self.delta[l.index]
        for i in range(T - 1, -1, -1):
            sl = slice(i * n, (i + 1) * n)
            if i:
                L["prevCell"] = cell[(i - 1) * n:i * n].copy()
            L["c"] = cell[sl].copy()
            if i:
                L["prevState"] = out[(i - 1) * n:i * n].copy()
            L["h"] = out[sl].copy()
            ds, dc = gates_backward(self.ora, [sub["w" + g]["out"][sl] for g in "figo"],
                                    [sub["u" + g]["out"][sl] for g in "figo"], L["c"],
                                    L["prevCell"], delta[sl], L["dc"])
            dh = delta if i else None
            # wo, uo, wg, ug, wi, ui, wf, uf: the order of the Pascal loop
            for g, d in reversed(list(zip("figo", ds))):
                sub["w" + g]["delta"][sl] = d
                self._sub_backward(l, L, sub["w" + g], i, L["prevState"], 0, dh, i - 1)
                sub["u" + g]["delta"][sl] = d
                self._sub_backward(l, L, sub["u" + g], i, inp, i, sd, i)
            L["dc"] = dc

    # -- passes ------------------------------------------------------------------------
    def forward(self, x, truth=None, training=True):
        ora, B = self.ora, self.net.batch
        prev = _c(x).ravel()
        for l in self.net.layers:
            i = l.index
            if training:
                np.multiply(self.delta[i], f32(0), out=self.delta[i])
            out = self.out[i]
            if l.kind == "lstm":
                self._lstm_forward(l, prev, training)
            elif l.kind == "connected":
                self._fc_forward(l, prev, training)
            elif l.kind == "softmax":
                out[:] = ora.softmax_rows(_c(prev), l.in_size // l.groups, l.temperature)
                if truth is not None and not l.noloss:
                    d, e = ora.softmax_xent(out, _c(truth).ravel())
                    self.delta[i][:] = d
                    self.loss[i][:] = e
                    self.costs[i] = f32(ora.vssum(self.loss[i]))
            else:
                raise ValueError(l.kind)
            prev = out
        self.check_finite()

    def backward(self, x):
        for l in reversed(self.net.layers):
            i = l.index
            inp = _c(x).ravel() if i == 0 else self.out[i - 1]
            sd = None if i == 0 else self.delta[i - 1]
            if l.kind == "lstm":
                self._lstm_backward(l, inp, sd)
            elif l.kind == "connected":
                self._fc_backward(l, inp, sd)
            elif l.kind == "softmax" and sd is not None:
                sd[:] = self.delta[i] + sd
        self.check_finite()

    def update(self, lr, momentum, decay):
        B = self.net.batch
        lrb = f32(f32(lr) / f32(B))
        ndb = f32(-f32(decay) * f32(B))
        for l in self.net.layers[:-1]:
            sts = ([self.lstm[l.index]["sub"][g] for g in LSTM_GATES] if l.kind == "lstm"
                   else [self.st[l.index]] if l.index in self.st else [])
            for st in sts:
                self.ora.sgd_update(st["w"], st["wu"], st["b"], st["bu"], st.get("scales"),
                                    st.get("su"), float(lrb), float(ndb), momentum)
        self.check_finite()

    def reset_state(self):
        for L in self.lstm.values():
            for k in STATE:
                L[k] = np.zeros(L["n"], f32)

    # -- what a comparison reads --------------------------------------------------------
    def state(self):
        """name -> array: every layer's output and delta, an lstm layer's cell
        and five state buffers, and per (sub-)layer the parameters, update
        buffers, statistics and BN inputs.  A sub-layer's delta is scratch
        outside the slice written last (step 0)."""
        s = {}
        for l in self.net.layers:
            i = l.index
            s[f"{i}.out"], s[f"{i}.delta"] = self.out[i], self.delta[i]
            if l.kind == "lstm":
                L = self.lstm[i]
                for k in STATE + ("cell",):
                    s[f"{i}.{k}"] = L[k]
                for g, st in L["sub"].items():
                    for k, v in st.items():
                        if k == "delta":
                            s[f"{i}.{g}.delta0"] = v[:L["n"]]
                        elif k != "I":
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
