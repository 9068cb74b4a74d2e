"""CPU checker for the global average pool (TAvgPoolLayer, navgpoollayer.pas:
60-108) and for the networks that end in it (test infrastructure).

* ``forward``: out[p] = f32(ora.vssum(plane p)) / f32(n) — the oracle's
  restated vssum_avx2 (eight accumulators, fold, two pair adds, tail in index
  order), then one float32 division;
* ``backward``: sd[p*n + i] = f32(sd[p*n + i] + f32(d[p] / f32(n))): the
  quotient rounded once, then one add per element;
* ``AvgRefNet``: tests/_classifier_oracle.py's RefNet with the ``avgpool``
  layer and the ``shortcut`` layer of tests/_darknet_oracle.py's pass
  (gradient, then the two adds).  Every other layer is RefNet's own code, run
  on a one-layer view of the plan, so nothing of it is restated here."""
import numpy as np

from _classifier_oracle import RefNet, _c

f32 = np.float32


def forward(ora, x, planes, n):
    x = _c(x).reshape(planes, n)
    out = np.empty(planes, f32)
    fn = f32(n)
    for p in range(planes):
        out[p] = f32(ora.vssum(x[p])) / fn
    return out


def backward(sd, d, planes, n):
    """In place on sd (planes*n floats)."""
    q = (_c(d).ravel() / f32(n)).astype(f32)
    v = sd.reshape(planes, n)
    v[:] = (v + q[:, None]).astype(f32)


class _One:
    """One layer of a plan as a plan of its own (the layer keeps its index)."""

    def __init__(self, net, l):
        self.batch, self.layers = net.batch, [l]


class AvgRefNet(RefNet):
    OWN = ("avgpool", "shortcut")

    def _as(self, l, fn, *args):
        full, self.net = self.net, _One(self.net, l)
        try:
            return fn(self, *args)
        finally:
            self.net = full

    def _own_forward(self, l, prev, outs):
        B = self.net.batch
        if l.kind == "avgpool":
            return forward(self.ora, prev, B * l.c, l.h * l.w)
        return self.ora.shortcut(_c(prev), _c(outs[l.inputs[0]]), l.activation)

    def forward(self, x, truth=None, seeds=()):
        seeds = iter(seeds)
        prev = _c(x).ravel()
        for l in self.net.layers:
            i = l.index
            if l.kind in self.OWN:
                np.multiply(self.delta[i], f32(0), out=self.delta[i])
                self.out[i][:] = self._own_forward(l, prev, self.out)
            else:
                self._as(l, RefNet.forward, prev, truth,
                         [next(seeds)] if l.kind == "dropout" else ())
            prev = self.out[i]

    def backward(self, x):
        B = self.net.batch
        for l in reversed(self.net.layers):
            i = l.index
            sd = None if i == 0 else self.delta[i - 1]
            d = self.delta[i]
            if l.kind == "avgpool":
                if sd is not None:
                    backward(sd, d, B * l.c, l.h * l.w)
            elif l.kind == "shortcut":  # naddlayer.pas:924-949
                self.ora.gradient(self.out[i], l.activation, d)
                sd[:] = d + sd
                src = self.delta[l.inputs[0]]
                src[:] = src + d
            else:
                self._as(l, RefNet.backward, x)

    def infer(self, x):
        prev = _c(x).ravel()
        outs = []
        for l in self.net.layers:
            if l.kind in self.OWN:
                y = self._own_forward(l, prev, outs)
            else:
                y = self._as(l, RefNet.infer, prev)[0]
            outs.append(_c(y).ravel())
            prev = outs[-1]
        return outs
