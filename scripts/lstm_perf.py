#!/usr/bin/env python3
"""The LSTM layer's gate stage and a whole training pass, the fused path
against the reference's call sequence, in one process with the two sides
alternating (HIP events, warm-up, median of several windows; the spread is the
windows' (max - min) / median).

1. One step's gate stage, forward and backward, at N = 32 * 1024 (the sample's
   streams * outputs) and N = 3 * 5 (launch overhead alone): ``lstmGatesForward``
   / ``lstmGatesBackward`` against the literal call sequence of
   TLSTMLayer.forwardGPU / backwardGPU made of the existing kernels (addvv,
   ActivateArray, mulvv, fmavv, copy, DeriveArray; in the backward also the
   copies into the eight sub-layer deltas and the clamp that opens each
   sub-layer's backward, which the fused kernel folds into its stores).  us,
   launches per step, and for the fused kernel its algorithmic bytes per
   element (forward: 9 floats read, 4 written; backward: 12 read, 9 written)
   over time.
2. A whole training pass (forward with truth + backward) of lstm_cfg(batch=32,
   time_steps=16, inputs=256, hidden=1024, layers=3), ``lstm_fused=True``
   against ``False``, batch norm on and off.  Host-side issue time is part of
   both sides (the calls are made from Python).

Before anything is timed both sides' results are compared bit for bit at the
timed sizes.  One JSON line to stdout.

  python scripts/lstm_perf.py > profiles/lstm_perf.json
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tensorium_amd import darknet as dn  # noqa: E402
from tensorium_amd._abi import ACT  # noqa: E402
from tensorium_amd.nnhip import TNNHip  # noqa: E402

LOG, TANH = ACT["LOGISTIC"], ACT["TANH"]


class Counting:
    """Counts the backend calls made through it."""

    def __init__(self, hip):
        self._hip, self.calls = hip, 0

    def __getattr__(self, name):
        f = getattr(self._hip, name)

        def g(*a, **k):
            self.calls += 1
            return f(*a, **k)
        return g


def ab(sides, reps, windows, warmup=2):
    """sides: name -> callable.  Per side the median over windows of the mean
    time (ms) of reps calls, windows of the sides alternating, and the spread."""
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    return {k: {"ms": statistics.median(v),
                "spread": (max(v) - min(v)) / statistics.median(v)} for k, v in ms.items()}


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- the gate stage ---------------------------------------------------------------------

def gate_buffers(N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda lo, hi: torch.rand(N, device="cuda", generator=g) * (hi - lo) + lo  # noqa: E731
    b = {k: r(-3, 3) for k in ("wf", "wi", "wg", "wo", "uf", "ui", "ug", "uo")}
    b.update(c0=r(-2, 2), cell=r(-2, 2), cprev=r(-2, 2), delta=r(-3, 3), dc0=r(-2, 2))
    for k in ("c", "h", "cell_out", "out", "dc", "_f", "_i", "_g", "_o", "t1", "t2", "t3"):
        b[k] = torch.zeros(N, device="cuda")
    for k in "figo":
        b["dw" + k], b["du" + k] = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    return b


def literal_gates(hip, b, N):
    for g in "figo":
        hip.addvv(N, b["w" + g], 0, 1, b["u" + g], 0, 1, b["_" + g], 0, 1)
    hip.ActivateArray(N, b["_f"], 0, LOG)
    hip.ActivateArray(N, b["_i"], 0, LOG)
    hip.ActivateArray(N, b["_o"], 0, LOG)
    hip.ActivateArray(N, b["_g"], 0, TANH)


def literal_forward(hip, b, N):
    literal_gates(hip, b, N)
    hip.mulvv(N, b["_i"], 0, 1, b["_g"], 0, 1, b["t1"], 0, 1)
    hip.fmavv(N, b["c"], 0, 1, b["_f"], 0, 1, b["t1"], 0, 1, b["c"], 0, 1)
    hip.copy(N, b["c"], 0, 1, b["h"], 0, 1)
    hip.ActivateArray(N, b["h"], 0, TANH)
    hip.mulvv(N, b["_o"], 0, 1, b["h"], 0, 1, b["h"], 0, 1)
    hip.copy(N, b["c"], 0, 1, b["cell_out"], 0, 1)
    hip.copy(N, b["h"], 0, 1, b["out"], 0, 1)


def literal_backward(hip, b, N):
    literal_gates(hip, b, N)
    t1, t2, t3 = b["t1"], b["t2"], b["t3"]
    hip.copy(N, b["delta"], 0, 1, t3, 0, 1)
    hip.copy(N, b["cell"], 0, 1, t1, 0, 1)
    hip.ActivateArray(N, t1, 0, TANH)
    hip.mulvv(N, t3, 0, 1, b["_o"], 0, 1, t2, 0, 1)
    hip.DeriveArray(N, t1, 0, TANH, t2)
    hip.addvv(N, b["dc"], 0, 1, t2, 0, 1, t2, 0, 1)
    hip.copy(N, b["cell"], 0, 1, t1, 0, 1)
    hip.ActivateArray(N, t1, 0, TANH)
    hip.mulvv(N, t3, 0, 1, t1, 0, 1, t1, 0, 1)
    hip.DeriveArray(N, b["_o"], 0, LOG, t1)
    for g, other, act in (("o", None, None), ("g", "_i", TANH), ("i", "_g", LOG),
                          ("f", "cprev", LOG)):
        if other is not None:
            hip.mulvv(N, t2, 0, 1, b[other], 0, 1, t1, 0, 1)
            hip.DeriveArray(N, b["_" + g], 0, act, t1)
        for side in "wu":
            hip.copy(N, t1, 0, 1, b["d" + side + g], 0, 1)
            hip.clamp(N, 1.0, b["d" + side + g], b["d" + side + g])
    hip.mulvv(N, t2, 0, 1, b["_f"], 0, 1, t1, 0, 1)
    hip.copy(N, t1, 0, 1, b["dc"], 0, 1)


def fused_forward(hip, b, N):
    hip.lstmGatesForward(N, [b["w" + g] for g in "figo"], [b["u" + g] for g in "figo"], b["c"],
                         b["h"], b["cell_out"], b["out"])


def fused_backward(hip, b, N):
    hip.lstmGatesBackward(N, [b["w" + g] for g in "figo"], [b["u" + g] for g in "figo"],
                          b["cell"], b["cprev"], b["delta"], b["dc"],
                          [b["dw" + g] for g in "figo"], [b["du" + g] for g in "figo"])


def gate_stage(hip, N, reps, windows):
    A, B = gate_buffers(N, 1), gate_buffers(N, 1)
    outs = {"forward": ("c", "h", "cell_out", "out"),
            "backward": ("dc",) + tuple("d" + s + g for s in "wu" for g in "figo")}
    row = {"N": N}
    for name, fused, literal, by in (("forward", fused_forward, literal_forward, 52),
                                     ("backward", fused_backward, literal_backward, 84)):
        for b in (A, B):   # the in / out operands from the same start
            b["c"].copy_(b["c0"])
            b["dc"].copy_(b["dc0"])
        cnt = Counting(hip)
        fused(hip, A, N)
        literal(cnt, B, N)
        torch.cuda.synchronize()
        if not all(same_bits(A[k], B[k]) for k in outs[name]):
            raise SystemExit(f"gate stage {name} N={N}: the two sides differ")
        t = ab({"fused": lambda: fused(hip, A, N), "literal": lambda: literal(hip, B, N)}, reps,
               windows)
        row[name] = {
            "fused_us": round(t["fused"]["ms"] * 1e3, 2),
            "literal_us": round(t["literal"]["ms"] * 1e3, 2),
            "fused_spread": round(t["fused"]["spread"], 3),
            "literal_spread": round(t["literal"]["spread"], 3),
            "fused_launches": 1, "literal_launches": cnt.calls,
            "fused_bytes_per_element": by,
            "fused_tbs": round(by * N / t["fused"]["ms"] / 1e9, 4)}
    return row


# ---- a whole training pass ----------------------------------------------------------------

def net_state(m):
    s = list(m.out) + list(m.delta)
    for L in m.lstm.values():
        s += [L[k] for k in ("c", "h", "dc", "prevCell", "prevState", "cell", "w_wu", "u_wu")]
        for st in L["sub"].values():
            s += [st["out"], st["bu"]] + [st[k] for k in ("su", "rm", "rv") if k in st]
    s += [st["wu"] for st in m.fc.values()]
    return s


def training_pass(hip, bn, batch, steps, inputs, hidden, layers, reps, windows):
    net = dn.Network(dn.parse_cfg(dn.lstm_cfg(batch, steps, inputs, hidden, layers, bool(bn))))
    params = dn.random_params(net, seed=3)
    rng = np.random.default_rng(3)
    B = net.batch
    x = torch.from_numpy(rng.uniform(-1, 1, (B, inputs)).astype(np.float32)).cuda()
    t = np.zeros((B, inputs), np.float32)
    t[np.arange(B), rng.integers(0, inputs, B)] = 1
    truth = torch.from_numpy(t).cuda()
    models, calls = {}, {}
    for name, fused in (("fused", True), ("literal", False)):
        cnt = Counting(hip)
        m = dn.HipDarknetTrain(cnt, net, params, torch, lstm_fused=fused)
        m.forward(x, truth)
        m.backward(x)
        calls[name] = cnt.calls
        m.hip = hip
        models[name] = m
    torch.cuda.synchronize()
    a, b = net_state(models["fused"]), net_state(models["literal"])
    if not all(same_bits(p, q) for p, q in zip(a, b)):
        raise SystemExit(f"training pass bn={bn}: the two sides differ")

    def one(m):
        def fn():
            m.forward(x, truth)
            m.backward(x)
        return fn

    r = ab({k: one(m) for k, m in models.items()}, reps, windows, warmup=1)
    return {"batch_normalize": int(bn), "rows": B, "streams": batch, "time_steps": steps,
            "fused_ms": round(r["fused"]["ms"], 3), "literal_ms": round(r["literal"]["ms"], 3),
            "fused_spread": round(r["fused"]["spread"], 3),
            "literal_spread": round(r["literal"]["spread"], 3),
            "fused_backend_calls": calls["fused"], "literal_backend_calls": calls["literal"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[32 * 1024, 3 * 5])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--time-steps", type=int, default=16)
    ap.add_argument("--inputs", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    hip = TNNHip(0)
    gates = [gate_stage(hip, n, 20, 7) for n in a.sizes]
    passes = [training_pass(hip, bn, a.batch, a.time_steps, a.inputs, a.hidden, a.layers, a.reps,
                            a.windows) for bn in (1, 0)]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "gate_stage": gates,
                      "training_pass": passes}))


if __name__ == "__main__":
    main()
