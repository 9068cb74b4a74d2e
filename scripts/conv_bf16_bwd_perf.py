#!/usr/bin/env python3
"""The 75 YOLOv3-416 conv layers' backward at batch 8, with state_delta,
through convBackward (the fp32 path at its default options) and
convBackwardBf16 (dW and dX on the bf16 MFMA), one process.

LINEAR activation, so the in-place delta preparation leaves delta as it is
from call to call; both paths run the same fp32 preparation (Derivative + bias
sums).  "bf16_dw" is convBackwardBf16 without state_delta: the preparation and
dW alone, so bf16 - bf16_dw is dX's share.

Each layer is warmed on every path, then timed `rounds` times, the paths
alternating inside a round: `reps` back-to-back calls between two device
events.  A path's total of a round is the sum of its 75 layer times; the
spread of a total is max - min over the rounds.  Writes per-layer and total
times, the spreads, and the per-class sums (output plane side, kernel size,
stride) as JSON.

  python scripts/conv_bf16_bwd_perf.py [--out profiles/conv_bf16_bwd_perf.json]
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

PATHS = ("fp32", "bf16", "bf16_dw")


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "conv_bf16_bwd_perf.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conv_bf16_bwd_perf: no GPU; nothing is measured without one")
    hip = TNNHip(0)
    B, layers, lin = a.batch, [], ACT["LINEAR"]
    for s in yolov3_conv_table()[:a.layers]:
        rnd = lambda *n: torch.rand(*n, device="cuda") * 0.2 - 0.1  # noqa: E731
        x, w = rnd(B, s.c, s.h, s.h), rnd(s.filters, s.K)
        out, d = rnd(B, s.filters, s.N), rnd(B, s.filters, s.N)
        bu, wu, sd = rnd(s.filters), torch.zeros_like(w), torch.zeros_like(x)
        ws = torch.empty(B * s.K * s.N, device="cuda")
        head = (B, s.c, s.h, s.h, x, w, s.filters, s.size, s.stride, s.pad)
        paths = {
            "fp32": lambda: hip.convBackward(*head, 1, lin, out, d, bu, wu, ws, sd),  # noqa: B023
            "bf16": lambda: hip.convBackwardBf16(*head, lin, out, d, bu, wu, sd),  # noqa: B023
            "bf16_dw": lambda: hip.convBackwardBf16(*head, lin, out, d, bu, wu, None),  # noqa: B023
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
        layers.append({"layer": s.index, "shape": f"{s.c}x{s.h} k{s.size}s{s.stride}->{s.filters}",
                       "class": f"{s.out_h}^2 {s.size}x{s.size}" + (" s2" if s.stride == 2 else ""),
                       "filters": s.M, "K": s.K, "R": s.N * B, "gflop": 2 * s.flops * B / 1e9,
                       "ms": ms})
        del x, w, out, d, bu, wu, sd, ws
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
        l["bf16_tflops"] = round(l.pop("gflop") / med["bf16"], 1)
        c = res["classes"].setdefault(l["class"], dict({"layers": 0}, **{k + "_ms": 0.0
                                                                         for k in PATHS}))
        c["layers"] += 1
        for k in PATHS:
            c[k + "_ms"] += med[k]
    for c in res["classes"].values():
        for k in PATHS:
            c[k + "_ms"] = round(c[k + "_ms"], 4)
        c["bf16_over_fp32"] = round(c["bf16_ms"] / c["fp32_ms"], 3)
    res["bf16_over_fp32"] = round(res["total_ms"]["bf16"] / res["total_ms"]["fp32"], 3)
    res["layers"] = layers
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: res[k] for k in ("total_ms", "spread_ms", "bf16_over_fp32", "classes")}))
    hip.close()


if __name__ == "__main__":
    main()
