"""The recurrent layers of the darknet drivers: ``_LstmLayers`` (TLSTMLayer,
nlstmlayer.pas:876-1294) and ``_RnnLayers`` (TRNNLayer, nrnnlayer.pas:148-257,
345-400), mixins of ``drivers._Driver``.  Each holds its layer's own step
logic; every sub-layer is a connected layer of ``connected.py``, called one
step at a time.  The driver supplies ``hip``, ``net``, ``out``, ``delta`` (in
training), the upload ``_t`` and the zeros ``_z``, and ``blocks``: the
parameter blocks of the sub-layers by (layer index, sub-layer name).
"""
from __future__ import annotations

from .._abi import ACT
from . import connected as fc
from .connected import at
from .description import LSTM_GATES, RNN_SUBS


class _LstmLayers:
    """The lstm layers of a driver (TLSTMLayer.forwardGPU / backwardGPU /
    updateGPU, nlstmlayer.pas:876-1294), shared by HipDarknet and
    HipDarknetTrain.  Rows are [step][stream]; n = streams * outputs floats
    make one step's slice.

    State per layer, as the reference keeps it: ``c``, ``h``, ``dc``,
    ``prevCell``, ``prevState`` (n floats each; never cleared by a pass),
    ``cell`` and the layer's output (steps * n), and per sub-layer the state of
    a connected layer (``connected.state``), its output and delta steps * n
    long.  The four w* (and the four u*) sub-layers' weights, weight_updates,
    outputs and deltas are slices of one buffer each, in the order f, i, g, o,
    so a strided-batched GEMM can cover them.

    ``lstm_fused=False`` is the reference's call sequence, call for call
    through the existing TNNHip methods.  ``lstm_fused=True`` is the product
    path: one ``lstmGatesForward`` / ``lstmGatesBackward`` per step, and
    GEMMs batched only where every output element keeps its operands and its
    order of additions (the LSTM section)."""

    W, U = LSTM_GATES[:4], LSTM_GATES[4:]

    def _lstm_init(self, blocks, training):
        z = self._z
        self.lstm = {}
        for l in self.net.lstms():
            T = l.steps
            S = self.net.batch // T
            O, I = l.filters, l.in_size
            n = S * O
            L = {"S": S, "T": T, "n": n, "sub": {}, "cell": z(T * n)}
            for k in ("c", "h", "dc", "prevCell", "prevState"):
                L[k] = z(n)
            if not self.lstm_fused:
                for k in ("f", "i", "g", "o", "temp", "temp2", "temp3"):
                    L["_" + k] = z(n)
            for side, names, K in (("w", self.W, O), ("u", self.U, I)):
                L[side + "_w"] = z(4 * O * K)
                L[side + "_out"] = z(4 * T * n)
                if training:
                    L[side + "_wu"] = z(4 * O * K)
                    L[side + "_delta"] = z(4 * T * n)
                for q, g in enumerate(names):  # a gate's slices of the side's four buffers
                    b, p = blocks[l.index, g]
                    cut = lambda k, m: L[side + k][q * m:(q + 1) * m]  # noqa: E731
                    L["sub"][g] = fc.state(self._t, z, p, O, K, b.activation, l.bn, T * S, training,
                                           out=cut("_out", T * n), w=cut("_w", O * K),
                                           delta=cut("_delta", T * n) if training else None,
                                           wu=cut("_wu", O * K) if training else None)
            self.lstm[l.index] = L

    def reset_state(self):
        """Zero c, h, dc, prevCell and prevState of every lstm layer (no pass
        does: the reference carries them from call to call)."""
        for L in self.lstm.values():
            for k in ("c", "h", "dc", "prevCell", "prevState"):
                L[k].zero_()

    # -- forward ---------------------------------------------------------------
    def _lstm_forward(self, l, inp, training):
        hip, L = self.hip, self.lstm[l.index]
        S, T, n, O, I = L["S"], L["T"], L["n"], l.filters, l.in_size
        sub, out, cell = L["sub"], self.out[l.index], L["cell"]
        inp = inp.reshape(-1)
        if training:  # nlstmlayer.pas:901-911 (the layer's own delta: the caller)
            for g in LSTM_GATES:
                hip.fill(T * n, sub[g]["delta"], 0, 0.0, 1)
        if not self.lstm_fused:
            for i in range(T):
                off = i * n
                for g in self.W:
                    fc.forward(hip, sub[g], S, i, L["h"], 0, training)
                for g in self.U:
                    fc.forward(hip, sub[g], S, i, inp, i, training)
                for g, dst in zip("figo", ("_f", "_i", "_g", "_o")):
                    hip.addvv(n, sub["w" + g]["out"], off, 1, sub["u" + g]["out"], off, 1, L[dst],
                              0, 1)
                hip.ActivateArray(n, L["_f"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_i"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_o"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_g"], 0, ACT["TANH"])
                hip.mulvv(n, L["_i"], 0, 1, L["_g"], 0, 1, L["_temp"], 0, 1)
                hip.fmavv(n, L["c"], 0, 1, L["_f"], 0, 1, L["_temp"], 0, 1, L["c"], 0, 1)
                hip.copy(n, L["c"], 0, 1, L["h"], 0, 1)
                hip.ActivateArray(n, L["h"], 0, ACT["TANH"])
                hip.mulvv(n, L["_o"], 0, 1, L["h"], 0, 1, L["h"], 0, 1)
                hip.copy(n, L["c"], 0, 1, cell, off, 1)
                hip.copy(n, L["h"], 0, 1, out, off, 1)
            return
        # the input-side products of every step and gate at once: an NT
        # product's element is one sdot of an input row and a weight row
        hip.gemmStridedBatched(False, True, T * S, O, I, 1.0, inp, 0, I, 0, L["u_w"], 0, I, O * I,
                               0.0, L["u_out"], 0, O, T * n, 4)
        for g in self.U:
            if l.bn:  # statistics are per step
                for i in range(T):
                    fc.bn_forward(hip, sub[g], S, i, training)
            else:     # a row's bias add does not depend on its step
                hip.forwardBias(T * n, sub[g]["out"], 0, O, sub[g]["b"], 1, T * S)
        for i in range(T):
            off = i * n
            hip.gemmStridedBatched(False, True, S, O, O, 1.0, L["h"], 0, O, 0, L["w_w"], 0, O,
                                   O * O, 0.0, L["w_out"], off, O, T * n, 4)
            for g in self.W:
                fc.bn_forward(hip, sub[g], S, i, training)
            hip.lstmGatesForward(n, [at(sub[g]["out"], off) for g in self.W],
                                 [at(sub[g]["out"], off) for g in self.U], L["c"], L["h"],
                                 at(cell, off), at(out, off))

    # -- backward ----------------------------------------------------------------
    def _lstm_backward(self, l, inp, sd):
        hip, L = self.hip, self.lstm[l.index]
        S, T, n, O, I = L["S"], L["T"], L["n"], l.filters, l.in_size
        sub, out, cell, delta = L["sub"], self.out[l.index], L["cell"], self.delta[l.index]
        inp = inp.reshape(-1)
        if not self.lstm_fused:
            for i in range(T - 1, -1, -1):
                off = i * n
                if i:
                    hip.copy(n, cell, off - n, 1, L["prevCell"], 0, 1)
                hip.copy(n, cell, off, 1, L["c"], 0, 1)
                if i:
                    hip.copy(n, out, off - n, 1, L["prevState"], 0, 1)
                hip.copy(n, out, off, 1, L["h"], 0, 1)
                for g, dst in zip("figo", ("_f", "_i", "_g", "_o")):
                    hip.addvv(n, sub["w" + g]["out"], off, 1, sub["u" + g]["out"], off, 1, L[dst],
                              0, 1)
                hip.ActivateArray(n, L["_f"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_i"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_o"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_g"], 0, ACT["TANH"])
                t1, t2, t3 = L["_temp"], L["_temp2"], L["_temp3"]
                hip.copy(n, delta, off, 1, t3, 0, 1)
                hip.copy(n, L["c"], 0, 1, t1, 0, 1)
                hip.ActivateArray(n, t1, 0, ACT["TANH"])
                hip.mulvv(n, t3, 0, 1, L["_o"], 0, 1, t2, 0, 1)
                hip.DeriveArray(n, t1, 0, ACT["TANH"], t2)
                hip.addvv(n, L["dc"], 0, 1, t2, 0, 1, t2, 0, 1)
                hip.copy(n, L["c"], 0, 1, t1, 0, 1)
                hip.ActivateArray(n, t1, 0, ACT["TANH"])
                hip.mulvv(n, t3, 0, 1, t1, 0, 1, t1, 0, 1)
                hip.DeriveArray(n, L["_o"], 0, ACT["LOGISTIC"], t1)
                dh = delta if i else None
                for g, other, act in (("o", None, None), ("g", "_i", "TANH"),
                                      ("i", "_g", "LOGISTIC"), ("f", "prevCell", "LOGISTIC")):
                    if other is not None:
                        hip.mulvv(n, t2, 0, 1, L[other], 0, 1, t1, 0, 1)
                        hip.DeriveArray(n, L["_" + g], 0, ACT[act], t1)
                    hip.copy(n, t1, 0, 1, sub["w" + g]["delta"], off, 1)
                    fc.backward(hip, sub["w" + g], S, i, L["prevState"], 0, dh, i - 1)
                    hip.copy(n, t1, 0, 1, sub["u" + g]["delta"], off, 1)
                    fc.backward(hip, sub["u" + g], S, i, inp, i, sd, i)
                hip.mulvv(n, t2, 0, 1, L["_f"], 0, 1, t1, 0, 1)
                hip.copy(n, t1, 0, 1, L["dc"], 0, 1)
            return
        for i in range(T - 1, -1, -1):
            off = i * n
            if i == 0 and T > 1:  # the copies of step 1; step 0 makes none (stale operands)
                hip.copy(n, cell, 0, 1, L["prevCell"], 0, 1)
                hip.copy(n, out, 0, 1, L["prevState"], 0, 1)
            cprev = at(cell, off - n) if i else L["prevCell"]
            hprev, hoff = (out, off - n) if i else (L["prevState"], 0)
            hip.lstmGatesBackward(n, [at(sub[g]["out"], off) for g in self.W],
                                  [at(sub[g]["out"], off) for g in self.U], at(cell, off), cprev,
                                  at(delta, off), L["dc"],
                                  [at(sub[g]["delta"], off) for g in self.W],
                                  [at(sub[g]["delta"], off) for g in self.U])
            for g in LSTM_GATES:
                fc.bn_backward(hip, sub[g], S, i, False)
            # the dW products: four outputs each, one operand shared
            hip.gemmStridedBatched(True, False, O, O, S, 1.0, L["w_delta"], off, O, T * n, hprev,
                                   hoff, O, 0, 1.0, L["w_wu"], 0, O, O * O, 4)
            hip.gemmStridedBatched(True, False, O, I, S, 1.0, L["u_delta"], off, O, T * n, inp,
                                   i * S * I, I, 0, 1.0, L["u_wu"], 0, I, O * I, 4)
            if i:  # into the layer's own delta, slice i-1, in the reference's order
                for g in ("wo", "wg", "wi", "wf"):
                    hip.gemm(False, False, S, O, O, 1.0, sub[g]["delta"], off, O, sub[g]["w"], 0, O,
                             1.0, delta, off - n, O)
        if sd is not None:  # slice i of the layer below's delta takes step i's four products
            for g in ("uo", "ug", "ui", "uf"):
                hip.gemm(False, False, T * S, I, O, 1.0, sub[g]["delta"], 0, O, sub[g]["w"], 0, I,
                         1.0, sd, 0, I)
        hip.copy(n, cell, 0, 1, L["c"], 0, 1)
        hip.copy(n, out, 0, 1, L["h"], 0, 1)

    def _lstm_update(self, l, learning_rate, momentum, decay):
        for g in LSTM_GATES:  # TLSTMLayer.updateGPU's order (nlstmlayer.pas:1281-1288)
            fc.update(self.hip, self.lstm[l.index]["sub"][g], self.net.batch, learning_rate,
                      momentum, decay)


class _RnnLayers:
    """The rnn layers of a driver (TRNNLayer.forward / backward / update, the
    CPU path, nrnnlayer.pas:148-257, 345-400 — the reference's device path
    disagrees with it), beside ``_LstmLayers``.  Rows are
    [step][stream]; n = streams * hidden floats make one hidden slice, m =
    streams * outputs one output slice.

    State per layer: ``state`` ((steps + 1) * n, zero at construction; a
    training forward zeroes slice 0, an inference forward nothing) and the
    three connected sub-layers input, self, output (``connected.state``),
    outputs and deltas steps * n (steps * m) long.  The output sub-layer's
    output and delta ARE the layer's.

    ``rnn_fused=False`` is the reference's call sequence, call for call
    through the existing TNNHip methods, the whole-delta clamp of every
    sub-layer backward included.  ``rnn_fused=True`` is the product path: one
    ``rnnStateForward`` per step, ``rnnDeltaBackward`` for the clamp + derive
    (+ copy + clamp + derive), and products regrouped only where every output
    element keeps its operands and its order of additions (the RNN
    section)."""

    def _rnn_init(self, blocks, training):
        z = self._z
        self.rnn = {}
        for l in self.net.rnns():
            T = l.steps
            S = self.net.batch // T
            L = {"S": S, "T": T, "n": S * l.hidden, "m": S * l.filters,
                 "state": z((T + 1) * S * l.hidden), "sub": {}}
            for g in RNN_SUBS:
                b, p = blocks[l.index, g]
                own = g == "output"  # the layer's own buffers
                L["sub"][g] = fc.state(self._t, z, p, b.filters, b.in_size, b.activation, l.bn,
                                       T * S, training, out=self.out[l.index] if own else None,
                                       delta=self.delta[l.index] if own and training else None)
            self.rnn[l.index] = L

    def reset_state(self):
        """Zero every rnn layer's whole ``state`` (no inference pass does: the
        reference carries it from call to call), and the lstm layers' state."""
        for L in self.rnn.values():
            L["state"].zero_()
        super().reset_state()

    # -- forward ---------------------------------------------------------------
    def _rnn_forward(self, l, inp, training):
        hip, L = self.hip, self.rnn[l.index]
        S, T, n, m, H, O, I = L["S"], L["T"], L["n"], L["m"], l.hidden, l.filters, l.in_size
        si, ss, so = (L["sub"][g] for g in RNN_SUBS)
        state = L["state"]
        inp = inp.reshape(-1)
        if training:  # nrnnlayer.pas:241-246: delta.multiply(0), state.FillExt(0, 0, n)
            hip.scale(T * m, 0.0, so["delta"], 1)
            hip.scale(T * n, 0.0, ss["delta"], 1)
            hip.scale(T * n, 0.0, si["delta"], 1)
            hip.fill(n, state, 0, 0.0, 1)
        j0 = 1 if training else 0  # step i writes state[i + j0] (rnnStepForward's j)
        if not self.rnn_fused:
            for i in range(T):
                j = i + j0
                fc.forward(hip, si, S, i, inp, i, training)
                fc.forward(hip, ss, S, i, state, i, training)
                if not l.shortcut:
                    hip.fill(n, state, j * n, 0.0, 1)
                elif j != i:  # (j = i: the slice onto itself)
                    hip.copy(n, state, i * n, 1, state, j * n, 1)
                hip.addvv(n, state, j * n, 1, si["out"], i * n, 1, state, j * n, 1)
                hip.addvv(n, state, j * n, 1, ss["out"], i * n, 1, state, j * n, 1)
                fc.forward(hip, so, S, i, state, j, training)
            return
        # the input sub-layer's products of every step at once: an NT product's
        # element is one sdot of an input row and a weight row
        hip.gemm(False, True, T * S, H, I, 1.0, inp, 0, I, si["w"], 0, I, 0.0, si["out"], 0, H)
        if l.bn and not training:  # by the rolling statistics: per element, any grouping
            hip.normalize(H, T * n, T * S, si["rm"], 1, si["rv"], 1, si["out"], 0)
            hip.forwardScaleAdd(T * n, si["out"], 0, H, si["scales"], si["b"], 1, T * S)
        for i in range(T):
            off = i * n
            hip.gemm(False, True, S, H, H, 1.0, state, off, H, ss["w"], 0, H, 0.0, ss["out"], off,
                     H)
            if l.bn:  # training: the statistics are per step
                if training:
                    fc.bn_forward(hip, si, S, i, True, activate=False)
                fc.bn_forward(hip, ss, S, i, training, activate=False)
            hip.rnnStateForward(n, H, at(si["out"], off), None if l.bn else si["b"], si.act,
                                at(ss["out"], off), None if l.bn else ss["b"], ss.act,
                                at(state, off) if l.shortcut else None, at(state, off + j0 * n))
        # the output sub-layer after the loop: step i reads state[i + j0], which
        # step i alone writes and no later step changes (in inference the steps
        # of one call do not chain: step i + 1 reads state[i + 1], not this one)
        hip.gemm(False, True, T * S, O, H, 1.0, state, j0 * n, H, so["w"], 0, H, 0.0, so["out"], 0,
                 O)
        if not l.bn:
            hip.forwardBias(T * m, so["out"], 0, O, so["b"], 1, T * S)
        elif training:
            for i in range(T):
                fc.bn_forward(hip, so, S, i, True, activate=False)
        else:
            hip.normalize(O, T * m, T * S, so["rm"], 1, so["rv"], 1, so["out"], 0)
            hip.forwardScaleAdd(T * m, so["out"], 0, O, so["scales"], so["b"], 1, T * S)
        hip.ActivateArray(T * m, so["out"], 0, so.act)

    # -- backward ----------------------------------------------------------------
    def _rnn_backward(self, l, inp, sd):
        hip, L = self.hip, self.rnn[l.index]
        S, T, n, m, H, I = L["S"], L["T"], L["n"], L["m"], l.hidden, l.in_size
        si, ss, so = (L["sub"][g] for g in RNN_SUBS)
        state = L["state"]
        inp = inp.reshape(-1)
        fused = self.rnn_fused
        for i in range(T - 1, -1, -1):
            off, offm = i * n, i * m
            # one add over the forward's value (the shortcut term dropped, as
            # the reference drops it); state[i] below is still the forward's
            hip.addvv(n, si["out"], off, 1, ss["out"], off, 1, state, off + n, 1)
            if fused:
                hip.rnnDeltaBackward(m, at(so["delta"], offm), at(so["out"], offm), so.act)
            fc.backward(hip, so, S, i, state, i + 1, ss["delta"], i, clamp=not fused)
            if fused:  # without batch norm the slice is final here: the input
                # sub-layer's copy, clamp and derive ride along
                chain = not l.bn
                hip.rnnDeltaBackward(n, at(ss["delta"], off), at(ss["out"], off), ss.act,
                                     at(si["delta"], off) if chain else None,
                                     at(si["out"], off) if chain else None, si.act)
            fc.backward(hip, ss, S, i, state, i, ss["delta"] if i else None, i - 1,
                               clamp=not fused)
            if not fused or l.bn:
                hip.copy(n, ss["delta"], off, 1, si["delta"], off, 1)
            if fused and l.bn:
                hip.rnnDeltaBackward(n, at(si["delta"], off), at(si["out"], off), si.act)
            if i and l.shortcut:
                hip.addvv(n, ss["delta"], off - n, 1, ss["delta"], off, 1, ss["delta"], off - n, 1)
            fc.backward(hip, si, S, i, inp, i, None if fused else sd, i, clamp=not fused)
        if not fused:
            return
        if sd is not None:  # slice i of the layer below's delta takes step i's product alone
            hip.gemm(False, False, T * S, I, H, 1.0, si["delta"], 0, H, si["w"], 0, I, 1.0, sd, 0,
                     I)
        if l.bn and T > 1:
            # the reference clamps the whole delta at every step: a slice that
            # normalizeDelta pushed outside [-1, 1] is clamped by the next step
            # (and no further: clamping is idempotent).  Nothing reads slice i
            # after step i, so one clamp of slices 1 .. T-1 leaves the layer's
            # delta as the reference does; slice 0 is processed last
            hip.clamp((T - 1) * m, 1.0, so["delta"], so["delta"], 1, m)

    def _rnn_update(self, l, learning_rate, momentum, decay):
        for g in RNN_SUBS:  # TRNNLayer.update's order (nrnnlayer.pas:393-395)
            fc.update(self.hip, self.rnn[l.index]["sub"][g], self.net.batch, learning_rate,
                      momentum, decay)
