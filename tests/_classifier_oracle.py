"""CPU restatement of a classifier network's training (TNNet.forward /
backward / update over convolutional, maxpool, connected, dropout, softmax,
cost and logistic layers), composed from the oracle's restated calls
(conv_forward_train, conv_backward_bn, sgemm, add_bias, activate, gradient,
add_sums, softmax_rows, softmax_xent, sgd_update ...), tests/_pool_oracle.py
and tests/_heads_oracle.py.  State persists over steps, as the layers' does.

Layer semantics as HipDarknetTrain's docstring lists them; the connected
layer is oracle/tns_oracle_train.c's fc_forward / fc_backward call for call
(bnMomentum 0.05).  A dropout layer's output and delta ARE the layer
below's arrays (the same numpy objects)."""
import numpy as np

import _heads_oracle as ho
from _pool_oracle import maxpool_backward, maxpool_forward

f32 = np.float32
LOSS = ("softmax", "cost", "logistic")


def _c(a):
    return np.ascontiguousarray(a, f32)


class RefNet:
    def __init__(self, ora, net, params):
        self.ora, self.net = ora, net
        B = net.batch
        self.st = {}
        for l, p in zip(net.param_layers(), params):
            st = {"w": _c(p.weights).copy(), "b": _c(p.biases).copy(),
                  "wu": np.zeros(p.weights.size, f32), "bu": np.zeros(l.filters, f32)}
            if l.bn:
                st.update(scales=_c(p.scales).copy(), rm=_c(p.rolling_mean).copy(),
                          rv=_c(p.rolling_var).copy(), su=np.zeros(l.filters, f32))
                for k in ("mean", "var", "md", "vd"):
                    st[k] = np.zeros(l.filters, f32)
            self.st[l.index] = st
        self.out, self.delta = [], []
        for l in net.layers:
            alias = l.kind == "dropout" and l.index > 0
            self.out.append(self.out[-1] if alias else np.zeros(B * l.out_size, f32))
            self.delta.append(self.delta[-1] if alias else np.zeros(B * l.out_size, f32))
        self.rnd = {l.index: np.zeros(B * l.out_size, f32)
                    for l in net.layers if l.kind == "dropout"}
        self.loss = {l.index: np.zeros(B * l.out_size, f32)
                     for l in net.layers if l.kind in ("softmax", "logistic")}
        self.costs = {l.index: f32(0) for l in net.layers if l.kind in LOSS}
        self.indexes = {}

    # -- connected ---------------------------------------------------------
    def _fc_forward(self, l, prev, training):
        ora, B, st = self.ora, self.net.batch, self.st[l.index]
        O, I = l.filters, l.in_size
        out = self.out[l.index]
        ora.sgemm(False, True, B, O, I, 1.0, _c(prev), I, st["w"], I, 0.0, out, O)
        if l.bn:
            if training:
                m, v, x, xn = ora.batch_norm(out, B, O, 1, st["scales"], st["b"], st["rm"],
                                             st["rv"], f32(0.05), True)
                st.update(mean=m, var=v, x=x, xn=xn)
            else:
                ora.normalize(out, B, O, 1, st["rm"], st["rv"])
                ora.forward_scale(out, B, O, 1, st["scales"])
                ora.add_bias(out, st["b"], O, 1, B)
        else:
            ora.add_bias(out, st["b"], O, 1, B)
        ora.activate(out, l.activation)

    def _fc_backward(self, l, inp, sd):
        ora, B, st = self.ora, self.net.batch, self.st[l.index]
        O, I = l.filters, l.in_size
        d = self.delta[l.index]
        ora._lib2().ora_clamp(ora._p(d), d.size, -1.0, 1.0)
        ora.gradient(self.out[l.index], l.activation, d)
        ora.add_sums(st["bu"], d, B, O, 1)
        if l.bn:
            ora.add_dots(st["su"], st["xn"], d, B, O, 1)
            ora.forward_scale(d, B, O, 1, st["scales"])
            st["md"], st["vd"] = ora.mean_var_delta(d, st["x"], st["mean"], st["var"], B, O, 1)
            ora.normalize_delta(st["x"], st["mean"], st["var"], st["md"], st["vd"], d, B, O, 1)
        ora.sgemm(True, False, O, I, B, 1.0, d, O, _c(inp), I, 1.0, st["wu"], I)
        if sd is not None:
            ora.sgemm(False, False, B, I, O, 1.0, d, O, st["w"], I, 1.0, sd, I)

    # -- passes -------------------------------------------------------------
    def forward(self, x, truth=None, seeds=()):
        ora, net, B = self.ora, self.net, self.net.batch
        seeds = iter(seeds)
        prev = _c(x).ravel()
        for l in net.layers:
            i = l.index
            if l.kind == "dropout":
                if i == 0:
                    self.out[0] = prev
                out = self.out[i]
                self.rnd[i], dst = ho.dropout_forward(next(seeds), l.probability, l.scale, out)
                out[:] = dst
                prev = out
                continue
            # cuda.scale(delta.size(), 0, delta, 1) (nnet.pas:291): a multiply,
            # so a negative element becomes -0.0, which a pool's backward keeps
            np.multiply(self.delta[i], f32(0), out=self.delta[i])
            out = self.out[i]
            if l.kind == "convolutional":
                st = self.st[i]
                p4 = prev.reshape(B, l.c, l.h, l.w)
                if l.bn:
                    y, m, v, xs, xn = ora.conv_forward_train(
                        p4, st["w"].ravel(), l.filters, l.size, l.stride, l.pad, l.activation,
                        st["scales"], st["b"], st["rm"], st["rv"], 0.1, True)
                    st.update(mean=m, var=v, x=xs.ravel(), xn=xn.ravel())
                else:
                    y = ora.conv_forward(p4, st["w"].ravel(), st["b"], l.filters, l.size,
                                         l.stride, l.pad, l.activation)
                out[:] = y.ravel()
            elif l.kind == "maxpool":
                y, self.indexes[i] = maxpool_forward(prev.reshape(B, l.c, l.h, l.w), l.size,
                                                     l.stride_x, l.stride_y, l.pad)
                out[:] = y.ravel()
            elif l.kind == "connected":
                self._fc_forward(l, prev, True)
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
            elif l.kind == "logistic":
                out[:] = prev
                ora.activate(out, l.activation)
                if truth is not None:
                    d, e = ho.cross_entropy_logistic(out, _c(truth).ravel())
                    self.delta[i][:] = d
                    self.loss[i][:] = e
                    self.costs[i] = f32(ora.vssum(self.loss[i]))
            else:
                raise ValueError(l.kind)
            prev = out

    def backward(self, x):
        ora, net, B = self.ora, self.net, self.net.batch
        for l in reversed(net.layers):
            i = l.index
            inp = _c(x).ravel() if i == 0 else self.out[i - 1]
            sd = None if i == 0 else self.delta[i - 1]
            d = self.delta[i]
            if l.kind == "convolutional":
                st = self.st[i]
                in4 = inp.reshape(B, l.c, l.h, l.w)
                if l.bn:
                    st["md"], st["vd"] = ora.conv_backward_bn(
                        in4, st["w"].ravel(), l.filters, l.size, l.stride, l.pad, l.activation,
                        self.out[i], d, st["scales"], st["x"], st["xn"], st["mean"], st["var"],
                        st["su"], st["wu"], sd)
                else:
                    ora.conv_backward(in4, st["w"].ravel(), l.filters, l.size, l.stride, l.pad,
                                      l.activation, self.out[i], d, st["bu"], st["wu"], sd)
            elif l.kind == "maxpool" and sd is not None:
                maxpool_backward(sd, self.indexes[i], d)
            elif l.kind == "connected":
                self._fc_backward(l, inp, sd)
            elif l.kind == "dropout" and sd is not None:
                sd[:] = ho.dropout_backward(l.probability, l.scale, sd, self.rnd[i])
            elif l.kind in ("softmax", "logistic") and sd is not None:
                sd[:] = d + sd
            elif l.kind == "cost" and sd is not None:   # axpy: one fused multiply-add
                sd[:] = (f32(l.scale).astype(np.float64) * d.astype(np.float64)
                         + sd.astype(np.float64)).astype(f32)

    def update(self, lr, momentum, decay):
        B = self.net.batch
        lrb = f32(f32(lr) / f32(B))
        ndb = f32(-f32(decay) * f32(B))
        for l in self.net.layers[:-1]:
            st = self.st.get(l.index)
            if st is not None:
                self.ora.sgd_update(st["w"], st["wu"], st["b"], st["bu"], st.get("scales"),
                                    st.get("su"), float(lrb), float(ndb), momentum)

    def cost(self):
        r = f32(0)
        for i in sorted(self.costs):
            r = f32(r + self.costs[i])
        return float(f32(r / f32(len(self.costs))))

    def infer(self, x):
        """Inference forward: BN-folded convolutions (as oracle.darknet_forward),
        rolling statistics in connected layers, dropout a no-op."""
        ora, net, B = self.ora, self.net, self.net.batch
        prev = _c(x).ravel()
        outs = []
        for l in net.layers:
            i = l.index
            if l.kind == "convolutional":
                st = self.st[i]
                w, b = st["w"].ravel().copy(), st["b"].copy()
                if l.bn:
                    ora.lib().ora_fuse_batchnorm(l.filters, l.c * l.size * l.size, ora._p(w),
                                                 ora._p(b), ora._p(st["scales"]), ora._p(st["rm"]),
                                                 ora._p(st["rv"]))
                y = ora.conv_forward(prev.reshape(B, l.c, l.h, l.w), w, b, l.filters, l.size,
                                     l.stride, l.pad, l.activation).ravel()
            elif l.kind == "maxpool":
                y = maxpool_forward(prev.reshape(B, l.c, l.h, l.w), l.size, l.stride_x,
                                    l.stride_y, l.pad)[0].ravel()
            elif l.kind == "connected":
                self._fc_forward(l, prev, False)
                y = self.out[i].copy()
            elif l.kind == "dropout":
                y = prev
            elif l.kind == "softmax":
                y = ora.softmax_rows(_c(prev), l.in_size // l.groups, l.temperature)
            elif l.kind == "logistic":
                y = ora.activate(prev.copy(), l.activation)
            else:
                raise ValueError(l.kind)
            outs.append(_c(y))
            prev = outs[-1]
        return outs
