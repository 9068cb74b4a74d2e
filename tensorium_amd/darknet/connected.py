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

The state also says which path the layer's three products take
(``product_nt`` / ``product_tn`` / ``product_nn``, the only place that
chooses): fp32 ``gemm`` by default; with ``bf16`` set (the drivers'
``connected_precision="bf16"``) ``gemmBf16``, and ``gemmBf16NTPacked`` for the
forward when the state holds the packed weights ``wp`` in place of ``w``
(inference: packed once at construction, the fp32 copy dropped).  Everything
else stays fp32 on either path.
"""
from __future__ import annotations

import numpy as np

BN_MOMENTUM = np.float32(0.05)  # bnMomentum (nconnectedlayer.pas:67), single arithmetic


def at(t, off):  # a raw device pointer off floats into t
    return t.data_ptr() + 4 * off


class State(dict):
    """The buffers by name, so that iterating it gives tensors only; ``O``,
    ``I`` and ``act`` are attributes, which ``st["O"]`` reads as well."""
    __slots__ = ("O", "I", "act", "bf16")

    def __init__(self, O, I, act, bf16=False, **buffers):
        super().__init__(**buffers)
        self.O, self.I, self.act, self.bf16 = O, I, act, bf16

    def __missing__(self, key):
        if key in self.__slots__:
            return getattr(self, key)
        raise KeyError(key)


def state(t, z, p, O, I, act, bn, rows, training, out=None, delta=None, w=None, wu=None,
          hip=None, precision="fp32"):
    """A connected (sub-)layer's device state from its parameter block ``p``.
    ``t`` uploads a NumPy array as float32, ``z(n)`` gives n device zeros;
    ``rows``: steps * streams.  What the owner keeps in buffers of its own is
    passed in: ``out`` / ``delta`` (a layer's output and delta; an lstm side's
    slab slices), ``w`` / ``wu`` (slab slices; ``w`` takes p's weights).
    ``precision="bf16"``: the products on the bf16 MFMA; in inference ``hip``
    packs the weights once and the state keeps ``wp`` instead of ``w``."""
    st = State(O, I, act, precision == "bf16", b=t(p.biases),
               out=z(rows * O) if out is None else out)
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
    elif st.bf16:  # the weights never change: packed once, the fp32 copy dropped
        st["wp"] = hip.gemmBf16Pack(O, I, st.pop("w"))
    return st


def product_nt(hip, st, rows, inp, in_off, out_off):
    """out[rows][O] (from float out_off) = inp[rows][I] (from in_off) . W^T."""
    O, I = st.O, st.I
    if "wp" in st:
        hip.gemmBf16NTPacked(rows, O, I, inp, in_off, I, st["wp"], False, st["out"], out_off, O)
    elif st.bf16:
        hip.gemmBf16(False, True, rows, O, I, inp, in_off, I, st["w"], 0, I, False, st["out"],
                     out_off, O)
    else:
        hip.gemm(False, True, rows, O, I, 1.0, inp, in_off, I, st["w"], 0, I, 0.0, st["out"],
                 out_off, O)


def product_tn(hip, st, rows, d_off, inp, in_off):
    """weight_updates[O][I] += delta[rows][O] (from d_off)^T . inp[rows][I]."""
    O, I = st.O, st.I
    if st.bf16:
        hip.gemmBf16(True, False, O, I, rows, st["delta"], d_off, O, inp, in_off, I, True,
                     st["wu"], 0, I)
    else:
        hip.gemm(True, False, O, I, rows, 1.0, st["delta"], d_off, O, inp, in_off, I, 1.0,
                 st["wu"], 0, I)


def product_nn(hip, st, rows, d_off, sd, sd_off):
    """sd[rows][I] (state.delta, from sd_off) += delta[rows][O] (from d_off) . W."""
    O, I = st.O, st.I
    if st.bf16:
        hip.gemmBf16(False, False, rows, I, O, st["delta"], d_off, O, st["w"], 0, I, True, sd,
                     sd_off, I)
    else:
        hip.gemm(False, False, rows, I, O, 1.0, st["delta"], d_off, O, st["w"], 0, I, 1.0, sd,
                 sd_off, I)


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
    product_nt(hip, st, S, inp, in_step * S * st.I, step * S * st.O)
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
    bn_backward(hip, st, S, step, clamp)
    off = step * S * st.O
    product_tn(hip, st, S, off, inp, in_step * S * st.I)
    if sd is not None:
        product_nn(hip, st, S, off, sd, sd_step * S * st.I)


def update(hip, st, batch, learning_rate, momentum, decay):
    """updateGPU's axpy / scale sequence fused (``sgdUpdate``) over a state
    dict, a convolution's included (it keeps the same keys)."""
    hip.sgdUpdate(st["w"], st["wu"], st["b"], st["bu"], learning_rate, batch, decay, momentum,
                  st.get("scales"), st.get("su"))
