"""One connected layer on the HIP backend: TConnectedLayer.forwardGPU /
backwardGPU / updateGPU (nconnectedlayer.pas:612-871), the only statement of
those call sequences in the drivers.  It serves the plain ``[connected]``
layer of both drivers (one step of ``batch`` rows), the eight gate sub-layers
of an lstm layer and the three sub-layers of an rnn layer (``steps`` steps of
``streams`` rows each, one step per call).

Forward (640-733): NT ``gemm``; with batch norm, in training, ``means``,
``variances``, the rolling statistics by ``scale`` / ``axpy`` (bnMomentum
0.05, line 67), ``copy`` to x, ``normalize``, ``copy`` to x_norm, in inference
``normalize`` by the rolling statistics, then ``forwardScaleAdd``; otherwise
``forwardBias``; ``ActivateArray``.  Backward (771-871): ``clamp(delta, 1)``
over the whole delta, ``DeriveArray``, ``backwardBias``, with batch norm
``addDots``, ``forwardScale``, ``meansAndVarsDelta``, ``normalizeDelta``, then
the TN ``gemm`` into weight_updates and the NN ``gemm`` into state.delta.

The state (``State``) is a dict of the layer's device buffers: ``w`` [O][I],
``b``, ``out``; batch-normalized ``scales rm rv``; in training ``wu bu delta``
and, batch-normalized, ``mean var x xn su md vd`` (one mean / variance pair,
overwritten each step).  Its attributes ``O`` (outputs), ``I`` (inputs) and
``act`` are the layer's own.  Rows are [step][stream]: S rows make one step, n =
S * O floats one step's slice of ``out`` / ``delta`` / ``x`` / ``xn``.
"""
from __future__ import annotations

import numpy as np

BN_MOMENTUM = np.float32(0.05)  # bnMomentum (nconnectedlayer.pas:67), single arithmetic


def at(t, off):  # a raw device pointer off floats into t
    return t.data_ptr() + 4 * off


class State(dict):
    """The buffers by name, so that iterating it gives tensors only; ``O``,
    ``I`` and ``act`` are attributes, which ``st["O"]`` reads as well."""
    __slots__ = ("O", "I", "act")

    def __init__(self, O, I, act, **buffers):
        super().__init__(**buffers)
        self.O, self.I, self.act = O, I, act

    def __missing__(self, key):
        if key in self.__slots__:
            return getattr(self, key)
        raise KeyError(key)


def state(t, z, p, O, I, act, bn, rows, training, out=None, delta=None, w=None, wu=None):
    """A connected (sub-)layer's device state from its parameter block ``p``.
    ``t`` uploads a NumPy array as float32, ``z(n)`` gives n device zeros;
    ``rows``: steps * streams.  What the owner keeps in buffers of its own is
    passed in: ``out`` / ``delta`` (a layer's output and delta; an lstm side's
    slab slices), ``w`` / ``wu`` (slab slices; ``w`` takes p's weights)."""
    st = State(O, I, act, b=t(p.biases), out=z(rows * O) if out is None else out)
    if w is None:
        st["w"] = t(p.weights)
    else:
        st["w"] = w
        w.copy_(t(p.weights).reshape(-1))
    if bn:
        st.update(scales=t(p.scales), rm=t(p.rolling_mean), rv=t(p.rolling_var))
    if training:
        st.update(wu=z(O * I) if wu is None else wu, bu=z(O),
                  delta=z(rows * O) if delta is None else delta)
        if bn:
            st.update(mean=z(O), var=z(O), x=z(rows * O), xn=z(rows * O), su=z(O), md=z(O),
                      vd=z(O))
    return st


def bn_forward(hip, st, S, step, training, activate=True):
    """What follows the product (nconnectedlayer.pas:654-733) on step's slice.
    activate=False: without the bias add (no batch norm) and the activation,
    which rnnStateForward makes."""
    O = st.O
    n = S * O
    out, off = st["out"], step * n
    if "scales" not in st:
        if activate:
            hip.forwardBias(n, out, off, O, st["b"], 1, S)
    else:
        if training:
            keep = float(np.float32(1) - BN_MOMENTUM)
            hip.means(n, O, S, out, off, st["mean"])
            hip.variances(n, O, S, out, off, st["mean"], st["var"])
            hip.scale(O, keep, st["rm"], 1)
            hip.axpy(O, float(BN_MOMENTUM), st["mean"], 0, 1, st["rm"], 0, 1)
            hip.scale(O, keep, st["rv"], 1)
            hip.axpy(O, float(BN_MOMENTUM), st["var"], 0, 1, st["rv"], 0, 1)
            hip.copy(n, out, off, 1, st["x"], off, 1)
            hip.normalize(O, n, S, st["mean"], 1, st["var"], 1, out, off)
            hip.copy(n, out, off, 1, st["xn"], off, 1)
        else:
            hip.normalize(O, n, S, st["rm"], 1, st["rv"], 1, out, off)
        hip.forwardScaleAdd(n, out, off, O, st["scales"], st["b"], 1, S)
    if activate:
        hip.ActivateArray(n, out, off, st.act)


def forward(hip, st, S, step, inp, in_step, training):
    """Step ``step`` from slice ``in_step`` of ``inp`` (S rows of I floats)."""
    O, I = st.O, st.I
    hip.gemm(False, True, S, O, I, 1.0, inp, in_step * S * I, I, st["w"], 0, I, 0.0, st["out"],
             step * S * O, O)
    bn_forward(hip, st, S, step, training)


def bn_backward(hip, st, S, step, clamp=True):
    """Up to the two products (nconnectedlayer.pas:771-821).  clamp=False:
    lstmGatesBackward stored the slice clamped already (rnnDeltaBackward:
    clamped and derived)."""
    O = st.O
    n = S * O
    d, off = st["delta"], step * n
    if clamp:
        hip.clamp(d.numel(), 1.0, d, d)
        # (the slice's own delta: with an lstm gate's LINEAR it multiplies by one)
        hip.DeriveArray(n, st["out"], off, st.act, at(d, off))
    hip.backwardBias(O, st["bu"], n, d, off, 1, S)
    if "scales" in st:
        hip.addDots(n, O, S, st["xn"], d, off, st["su"])
        hip.forwardScale(n, d, off, O, st["scales"], 1, S)
        hip.meansAndVarsDelta(n, O, S, d, st["x"], off, st["mean"], st["var"], st["md"], st["vd"])
        hip.normalizeDelta(n, O, S, d, st["x"], off, st["mean"], st["var"], st["md"], st["vd"])


def backward(hip, st, S, step, inp, in_step, sd, sd_step, clamp=True):
    """Step ``step``: weight_updates from slice ``in_step`` of ``inp``, and
    into slice ``sd_step`` of ``sd`` (state.delta) unless it is None."""
    O, I = st.O, st.I
    bn_backward(hip, st, S, step, clamp)
    d, off = st["delta"], step * S * O
    hip.gemm(True, False, O, I, S, 1.0, d, off, O, inp, in_step * S * I, I, 1.0, st["wu"], 0, I)
    if sd is not None:
        hip.gemm(False, False, S, I, O, 1.0, d, off, O, st["w"], 0, I, 1.0, sd, sd_step * S * I, I)


def update(hip, st, batch, learning_rate, momentum, decay):
    """updateGPU's axpy / scale sequence fused (``sgdUpdate``) over a state
    dict, a convolution's included (it keeps the same keys)."""
    hip.sgdUpdate(st["w"], st["wu"], st["b"], st["bu"], learning_rate, batch, decay, momentum,
                  st.get("scales"), st.get("su"))
