#!/usr/bin/env python3
"""The RNN layer's per-step elementwise stage and a whole training pass, the
fused path against the reference's call sequence, in one process with the two
sides alternating (HIP events, warm-up, median of several windows; the spread
is the windows' (max - min) / median).

1. One step's elementwise stage at N = 32 * 1024 (the sample's streams *
   hidden) and N = 3 * 5 (launch overhead alone), H = 1024 / 5, LEAKY:
   ``rnnStateForward`` against forwardBias x2, ActivateArray x2, fill, addvv
   x2 (without batch norm; with it the biases are null and the literal side
   loses its two forwardBias calls), and ``rnnDeltaBackward`` with delta2
   against clamp, DeriveArray, copy, clamp, DeriveArray (a slice's share: the
   reference clamps the whole delta, steps times as much).  us, launches per
   step, and for the fused kernel its algorithmic bytes per element (forward:
   2 floats read, 3 written, the bias rows apart; backward: 3 read, 2
   written) over time.
2. A whole training pass (forward with truth + backward) of rnn_cfg(batch=32,
   time_steps=16, inputs=256, hidden=1024, layers=3), ``rnn_fused=True``
   against ``False``, batch norm on and off.  Host-side issue time is part of
   both sides (the calls are made from Python).

Before anything is timed both sides' results are compared bit for bit at the
timed sizes.  One JSON line to stdout.

  python scripts/rnn_perf.py > profiles/rnn_perf.json
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

LEAKY = ACT["LEAKY"]


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


# ---- the elementwise stage ----------------------------------------------------------------

def step_buffers(N, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda n, lo, hi: torch.rand(n, device="cuda", generator=g) * (hi - lo) + lo  # noqa: E731
    b = dict(a0=r(N, -3, 3), b0=r(N, -3, 3), ab=r(H, -0.5, 0.5), bb=r(H, -0.5, 0.5),
             d0=r(N, -3, 3), out=r(N, -1, 1), out2=r(N, -1, 1))
    for k in ("a", "b", "next", "delta", "delta2"):
        b[k] = torch.zeros(N, device="cuda")
    return b


def reset(b):   # the in / out operands from the same start (the stage is not idempotent)
    b["a"].copy_(b["a0"])
    b["b"].copy_(b["b0"])
    b["delta"].copy_(b["d0"])


def fused_forward(hip, b, N, H):
    hip.rnnStateForward(N, H, b["a"], b["ab"], LEAKY, b["b"], b["bb"], LEAKY, None, b["next"])


def literal_forward(hip, b, N, H):
    for x, bias in (("a", "ab"), ("b", "bb")):
        hip.forwardBias(N, b[x], 0, H, b[bias], 1, N // H)
        hip.ActivateArray(N, b[x], 0, LEAKY)
    hip.fill(N, b["next"], 0, 0.0, 1)
    hip.addvv(N, b["next"], 0, 1, b["a"], 0, 1, b["next"], 0, 1)
    hip.addvv(N, b["next"], 0, 1, b["b"], 0, 1, b["next"], 0, 1)


def fused_backward(hip, b, N, H):
    hip.rnnDeltaBackward(N, b["delta"], b["out"], LEAKY, b["delta2"], b["out2"], LEAKY)


def literal_backward(hip, b, N, H):
    hip.clamp(N, 1.0, b["delta"], b["delta"])
    hip.DeriveArray(N, b["out"], 0, LEAKY, b["delta"])
    hip.copy(N, b["delta"], 0, 1, b["delta2"], 0, 1)
    hip.clamp(N, 1.0, b["delta2"], b["delta2"])
    hip.DeriveArray(N, b["out2"], 0, LEAKY, b["delta2"])


def step_stage(hip, N, H, reps, windows):
    A, B = step_buffers(N, H, 1), step_buffers(N, H, 1)
    outs = {"forward": ("a", "b", "next"), "backward": ("delta", "delta2")}
    row = {"N": N, "H": H}
    for name, fused, literal, by in (("forward", fused_forward, literal_forward, 20),
                                     ("backward", fused_backward, literal_backward, 20)):
        reset(A)
        reset(B)
        cnt = Counting(hip)
        fused(hip, A, N, H)
        literal(cnt, B, N, H)
        torch.cuda.synchronize()
        if not all(same_bits(A[k], B[k]) for k in outs[name]):
            raise SystemExit(f"step stage {name} N={N}: the two sides differ")
        # timed on whatever the slices hold by then: LEAKY and the clamp cost
        # the same on any value
        t = ab({"fused": lambda: fused(hip, A, N, H), "literal": lambda: literal(hip, B, N, H)},
               reps, windows)
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
    """What a pass leaves that anything reads: outputs, deltas, state, every
    update buffer and statistic, and slice 0 of the inner sub-layers' deltas."""
    s = list(m.out) + list(m.delta)
    for L in m.rnn.values():
        s.append(L["state"])
        for st in L["sub"].values():
            s += [st["out"], st["wu"], st["bu"], st["delta"][:L["S"] * st["O"]]]
            s += [st[k] for k in ("su", "rm", "rv", "x", "xn", "mean", "var") if k in st]
    s += [st["wu"] for st in m.fc.values()]
    return s


def training_pass(hip, bn, batch, steps, inputs, hidden, layers, reps, windows):
    net = dn.Network(dn.parse_cfg(dn.rnn_cfg(batch, steps, inputs, hidden, layers, bool(bn))),
                     rnn=True)
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
        m = dn.HipDarknetTrain(cnt, net, params, torch, rnn_fused=fused)
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
    ap.add_argument("--sizes", type=int, nargs="*", default=[32 * 1024, 1024, 3 * 5, 5],
                    help="N H pairs")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--time-steps", type=int, default=16)
    ap.add_argument("--inputs", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    hip = TNNHip(0)
    steps = [step_stage(hip, n, h, 20, 7) for n, h in zip(a.sizes[::2], a.sizes[1::2])]
    passes = [training_pass(hip, bn, a.batch, a.time_steps, a.inputs, a.hidden, a.layers, a.reps,
                            a.windows) for bn in (1, 0)]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "step_stage": steps,
                      "training_pass": passes}))


if __name__ == "__main__":
    main()
