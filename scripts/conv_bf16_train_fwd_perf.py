#!/usr/bin/env python3
"""The 75 YOLOv3-416 conv layers' training forward at batch 8, one process:

  fp32          convForwardTrain: the fp32 product, then the batch-norm chain
  bf16          convForwardTrainBf16: the product on the bf16 MFMA from the
                plain fp32 weights, then the same chain
  bf16_product  convForwardBf16Weights (zero bias, linear): that product alone
  packed        convBf16Pack + convForwardBf16 (zero bias, linear): the product
                as a training loop had to get it before, packing every step

so bf16 against fp32 is the layer's training forward, and bf16_product against
packed the product alone.  Every layer is run as a batch-normalized one.

Each layer is warmed on every path, then timed `rounds` times, the paths
alternating inside a round: `reps` back-to-back calls between two device
events.  A path's total of a round is the sum of its 75 layer times; the spread
of a total is max - min over the rounds.  Writes per-layer and total times, the
spreads, and the per-class sums (output plane side, kernel size, stride) as
JSON.

  python scripts/conv_bf16_train_fwd_perf.py [--out profiles/conv_bf16_train_fwd_perf.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tensorium_amd._abi import ACT  # noqa: E402
from tensorium_amd.nnhip import TNNHip  # noqa: E402
from tensorium_amd.yolo import yolov3_conv_table  # noqa: E402

PATHS = ("fp32", "bf16", "bf16_product", "packed")


def timed(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=30.0)
    ap.add_argument("--layers", type=int, default=75, help="the first n layers (rehearsals)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "conv_bf16_train_fwd_perf.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conv_bf16_train_fwd_perf: no GPU; nothing is measured without one")
    hip = TNNHip(0)
    B, layers, lin, leaky = a.batch, [], ACT["LINEAR"], ACT["LEAKY"]
    for s in yolov3_conv_table()[:a.layers]:
        rnd = lambda *n: torch.rand(*n, device="cuda") * 0.2 - 0.1  # noqa: E731
        z = lambda *n: torch.zeros(*n, device="cuda")  # noqa: E731
        F = s.filters
        x, w, out = rnd(B, s.c, s.h, s.h), rnd(F, s.K), z(B, F, s.N)
        sc, bi, rm, rv, zero = rnd(F) + 1.0, rnd(F), z(F), z(F) + 1.0, z(F)
        mean, var, xs, xn = z(F), z(F), z(B, F, s.N), z(B, F, s.N)
        ws = torch.empty(B * s.K * s.N, device="cuda")
        packed = hip.convBf16Pack(F, s.K, w)
        head = (B, s.c, s.h, s.h, x, w, F, s.size, s.stride, s.pad)
        bn = (leaky, sc, bi, rm, rv, 0.1, True, mean, var, xs, xn)

        def pack_forward():
            hip.convBf16Pack(F, s.K, w, packed)  # noqa: B023
            hip.convForwardBf16(B, s.c, s.h, s.h, x, packed, zero, F, s.size,  # noqa: B023
                                s.stride, s.pad, lin, out)  # noqa: B023
        paths = {
            "fp32": lambda: hip.convForwardTrain(*head, 1, *bn, ws, out),  # noqa: B023
            "bf16": lambda: hip.convForwardTrainBf16(*head, *bn, out),  # noqa: B023
            "bf16_product": lambda: hip.convForwardBf16Weights(  # noqa: B023
                B, s.c, s.h, s.h, x, w, zero, F, s.size, s.stride, s.pad, lin, out),  # noqa: B023
            "packed": pack_forward,
        }
        ms = {k: [] for k in paths}
        for run in paths.values():  # every shape warmed; the clock ramps under load
            t_end = time.perf_counter() + a.warm_ms / 1e3
            while time.perf_counter() < t_end:
                for _ in range(5):
                    run()
                torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, run in paths.items():
                ms[k].append(timed(run, a.reps))
        layers.append({"layer": s.index, "shape": f"{s.c}x{s.h} k{s.size}s{s.stride}->{F}",
                       "class": f"{s.out_h}^2 {s.size}x{s.size}" + (" s2" if s.stride == 2 else ""),
                       "filters": s.M, "K": s.K, "N": s.N * B, "gflop": 2 * s.flops * B / 1e9,
                       "ms": ms})
        del x, w, out, xs, xn, ws, packed
    res = {"batch": B, "reps": a.reps, "rounds": a.rounds, "total_ms": {}, "spread_ms": {},
           "classes": {}}
    for k in PATHS:
        totals = [sum(l["ms"][k][r] for l in layers) for r in range(a.rounds)]
        res["total_ms"][k] = round(sorted(totals)[a.rounds // 2], 4)
        res["spread_ms"][k] = round(max(totals) - min(totals), 4)
    for l in layers:
        med = {k: sorted(v)[a.rounds // 2] for k, v in l.pop("ms").items()}
        for k in PATHS:
            l[k + "_ms"] = round(med[k], 4)
        l["bf16_product_tflops"] = round(l.pop("gflop") / med["bf16_product"], 1)
        c = res["classes"].setdefault(l["class"], dict({"layers": 0}, **{k + "_ms": 0.0
                                                                         for k in PATHS}))
        c["layers"] += 1
        for k in PATHS:
            c[k + "_ms"] += med[k]
    for c in res["classes"].values():
        for k in PATHS:
            c[k + "_ms"] = round(c[k + "_ms"], 4)
        c["bf16_over_fp32"] = round(c["bf16_ms"] / c["fp32_ms"], 3)
    t = res["total_ms"]
    res["bf16_over_fp32"] = round(t["bf16"] / t["fp32"], 3)
    res["bf16_product_over_packed"] = round(t["bf16_product"] / t["packed"], 3)
    res["layers"] = layers
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: res[k] for k in ("total_ms", "spread_ms", "bf16_over_fp32",
                                          "bf16_product_over_packed", "classes")}))
    hip.close()


if __name__ == "__main__":
    main()
