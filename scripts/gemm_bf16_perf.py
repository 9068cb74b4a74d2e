#!/usr/bin/env python3
"""The connected layer's three products through tns_hip_gemm (fp32) and
tns_gemm_bf16 / tns_gemm_bf16_nt_packed, and whole passes of the nets they
serve under connected_precision "fp32" and "bf16", one process.

Shapes (rows S, inputs I, outputs O): the MNIST sample's connected layers at
its batch (bench_mnist: 784-64-64-64-64-32-10, batch 32; the 784 -> 64 and a
64 -> 64 layer) and the char-LSTM sample's gate sub-layers at 32 streams
(lstm_cfg: inputs 256, hidden 1024; the u side 256 -> 1024 and the w side
1024 -> 1024).  Per shape the forward (NT), weight_updates (TN, accumulate) and
state.delta (NN, accumulate) products, with the floating-point operations and
the least bytes each path must move, computed from the shape.

Nets: the MNIST connected net (batch 32, batch norm) and lstm_cfg(batch 32,
time_steps 4: 32 streams, 3 layers of 1024, batch norm): one HipDarknet forward
and one HipDarknetTrain step (forward with truth, backward, update).

Everything is warmed, then timed `rounds` times with the paths alternating
inside a round: `reps` back-to-back calls between two device events.  Reported:
the median over the rounds and the spread (max - min) over the rounds, in us.
Host-side issue time is part of every figure (the calls are made from Python).

  python scripts/gemm_bf16_perf.py [--out profiles/gemm_bf16_perf.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tensorium_amd import darknet as dn  # noqa: E402
from tensorium_amd.nnhip import TNNHip  # noqa: E402

SHAPES = {"mnist 784->64 @32": (32, 784, 64), "mnist 64->64 @32": (32, 64, 64),
          "lstm u 256->1024 @32": (32, 256, 1024), "lstm w 1024->1024 @32": (32, 1024, 1024)}
MNIST = ("[net]\nbatch=32\nwidth=784\nheight=1\nchannels=1\n"
         + "".join(f"[connected]\noutput={o}\nactivation={a}\nbatch_normalize=1\n"
                   for o, a in zip((64, 64, 64, 64, 32, 10), ("relu",) * 5 + ("linear",)))
         + "[softmax]\n")


def timed(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def rounds_of(paths, reps, rounds):
    """{path: {us, spread_us}} with the paths alternating inside each round."""
    for run in paths.values():
        timed(run, max(3, reps // 4))
    t = {k: [] for k in paths}
    for _ in range(rounds):
        for k, run in paths.items():
            t[k].append(timed(run, reps))
    return {k: {"us": round(statistics.median(v), 3), "spread_us": round(max(v) - min(v), 3)}
            for k, v in t.items()}


def products(hip, S, I, O, reps, rounds):
    g = torch.Generator(device="cuda").manual_seed(S + I + O)
    r = lambda *n: torch.rand(*n, device="cuda", generator=g) * 2 - 1  # noqa: E731
    x, w, d, out, wu, sd = r(S * I), r(O * I), r(S * O), r(S * O), r(O * I), r(S * I)
    wp = hip.gemmBf16Pack(O, I, w)
    res, F, T = {}, False, True
    forms = {
        "NT": dict(M=S, N=O, K=I, acc=0,
                   fp32=lambda: hip.gemm(F, T, S, O, I, 1.0, x, 0, I, w, 0, I, 0.0, out, 0, O),
                   bf16=lambda: hip.gemmBf16(F, T, S, O, I, x, 0, I, w, 0, I, F, out, 0, O),
                   bf16_packed=lambda: hip.gemmBf16NTPacked(S, O, I, x, 0, I, wp, F, out, 0, O)),
        "TN": dict(M=O, N=I, K=S, acc=1,
                   fp32=lambda: hip.gemm(T, F, O, I, S, 1.0, d, 0, O, x, 0, I, 1.0, wu, 0, I),
                   bf16=lambda: hip.gemmBf16(T, F, O, I, S, d, 0, O, x, 0, I, T, wu, 0, I)),
        "NN": dict(M=S, N=I, K=O, acc=1,
                   fp32=lambda: hip.gemm(F, F, S, I, O, 1.0, d, 0, O, w, 0, I, 1.0, sd, 0, I),
                   bf16=lambda: hip.gemmBf16(F, F, S, I, O, d, 0, O, w, 0, I, T, sd, 0, I)),
    }
    for form, f in forms.items():
        M, N, K, acc = f["M"], f["N"], f["K"], f["acc"]
        paths = {k: f[k] for k in ("fp32", "bf16", "bf16_packed") if k in f}
        # the NT paths against each other (the accumulating forms change their output)
        diff = None
        if form == "NT":
            paths["fp32"]()
            ref = out.clone()
            paths["bf16_packed"]()
            diff = float((out - ref).abs().max())
        a_el, b_el, c_el = M * K, K * N, M * N * (1 + acc)
        res[form] = {"M": M, "N": N, "K": K, "flop": 2 * M * N * K,
                     "min_bytes_fp32": 4 * (a_el + b_el + c_el),
                     "min_bytes_bf16_packed": 4 * (a_el + c_el) + 2 * b_el,
                     "max_abs_diff_packed_vs_fp32": diff, **rounds_of(paths, reps, rounds)}
    return res


def nets(hip, name, cfg, reps, rounds):
    net = dn.Network(dn.parse_cfg(cfg), rnn=True)
    params = dn.random_params(net, seed=3)
    shape = (net.batch, net.c, net.h, net.w) if net.c else (net.batch, net.inputs)
    x = torch.rand(shape, device="cuda")
    truth = torch.zeros(net.batch, net.layers[-1].out_size, device="cuda")
    truth[:, 0] = 1.0
    paths = {}
    for prec in ("fp32", "bf16"):
        inf = dn.HipDarknet(hip, net, params, torch, connected_precision=prec)
        tr = dn.HipDarknetTrain(hip, net, params, torch, connected_precision=prec)

        def step(tr=tr):
            tr.forward(x, truth)
            tr.backward(x)
            tr.update(1e-4, 0.9, 1e-4)
        paths[f"forward_{prec}"] = lambda inf=inf: inf.forward(x)
        paths[f"train_step_{prec}"] = step
    return {"net": name, **rounds_of(paths, reps, rounds)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--net-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gemm_bf16_perf.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gemm_bf16_perf: no GPU; nothing is measured without one")
    hip = TNNHip(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "net_reps": a.net_reps,
           "rounds": a.rounds, "unit": "us a call: median over the rounds; spread = max - min",
           "products": {k: products(hip, *s, a.reps, a.rounds) for k, s in SHAPES.items()},
           "nets": [nets(hip, "mnist connected 784-64x4-32-10 bn, batch 32", MNIST, a.net_reps,
                         a.rounds),
                    nets(hip, "lstm 3x1024 bn, inputs 256, 32 streams x 4 steps",
                         dn.lstm_cfg(32, 4, 256, 1024, 3, True), max(2, a.net_reps // 3),
                         a.rounds)]}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
