#!/usr/bin/env python3
"""The 75 YOLOv3-416 conv layers at batch 8 through convForward(fused=True)
(fp32 MFMA, the default path) and convForwardBf16 (bf16 MFMA), one process.

Each layer is warmed on both paths, then timed `rounds` times, the two paths
alternating inside a round: `reps` back-to-back calls between two device
events.  A path's total of a round is the sum of its 75 layer times; the
spread of a total is max - min over the rounds.  Writes per-layer and total
times, the spreads, and the per-class sums (output plane side, kernel size)
as JSON.  --tile forces TNS_OPT_CONV_BF16_TILE.

  python scripts/conv_bf16_perf.py [--out profiles/conv_bf16_perf.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tensorium_amd.nnhip import TNNHip  # noqa: E402
from tensorium_amd.yolo import yolov3_conv_table  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=30.0)
    ap.add_argument("--tile", type=int, default=-1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "conv_bf16_perf.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conv_bf16_perf: no GPU; nothing is measured without one")
    hip = TNNHip(0)
    hip.setConvBf16Tile(a.tile)
    B, layers = a.batch, []
    for s in yolov3_conv_table():
        x = torch.rand(B, s.c, s.h, s.h, device="cuda") * 2 - 1
        w = torch.rand(s.filters, s.K, device="cuda") * 0.2 - 0.1
        b = torch.rand(s.filters, device="cuda") * 0.2 - 0.1
        packed = hip.convBf16Pack(s.filters, s.K, w)
        out = torch.empty(B, s.filters, s.N, device="cuda")
        paths = {
            "fp32": lambda: hip.convForward(B, s.c, s.h, s.h, x, w, b, s.filters, s.size,  # noqa
                                            s.stride, s.pad, 1, s.activation, None, out,
                                            fused=True),
            "bf16": lambda: hip.convForwardBf16(B, s.c, s.h, s.h, x, packed, b, s.filters,  # noqa
                                                s.size, s.stride, s.pad, s.activation, out),
        }
        ms = {k: [] for k in paths}
        for run in paths.values():  # every shape warmed; the clock ramps under load
            t_end = time.perf_counter() + a.warm_ms / 1e3
            while time.perf_counter() < t_end:
                for _ in range(10):
                    run()
                torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, run in paths.items():
                ms[k].append(timed(run, a.reps))
        layers.append({"layer": s.index, "shape": f"{s.c}x{s.h} k{s.size}s{s.stride}->{s.filters}",
                       "class": f"{s.out_h}^2 {s.size}x{s.size}", "M": s.M, "N": s.N * B,
                       "K": s.K, "gflop": s.flops * B / 1e9, "ms": ms})
    res = {"batch": B, "reps": a.reps, "rounds": a.rounds, "tile": a.tile, "total_ms": {},
           "spread_ms": {}, "classes": {}}
    for k in ("fp32", "bf16"):
        totals = [sum(l["ms"][k][r] for l in layers) for r in range(a.rounds)]
        res["total_ms"][k] = round(sorted(totals)[a.rounds // 2], 4)
        res["spread_ms"][k] = round(max(totals) - min(totals), 4)
    for l in layers:
        med = {k: sorted(v)[a.rounds // 2] for k, v in l.pop("ms").items()}
        l["fp32_ms"], l["bf16_ms"] = round(med["fp32"], 4), round(med["bf16"], 4)
        l["bf16_tflops"] = round(l.pop("gflop") / med["bf16"], 1)
        c = res["classes"].setdefault(l["class"], {"layers": 0, "fp32_ms": 0.0, "bf16_ms": 0.0})
        c["layers"] += 1
        c["fp32_ms"] += med["fp32"]
        c["bf16_ms"] += med["bf16"]
    for c in res["classes"].values():
        c["fp32_ms"], c["bf16_ms"] = round(c["fp32_ms"], 4), round(c["bf16_ms"], 4)
        c["bf16_over_fp32"] = round(c["bf16_ms"] / c["fp32_ms"], 3)
    res["bf16_over_fp32"] = round(res["total_ms"]["bf16"] / res["total_ms"]["fp32"], 3)
    res["layers"] = layers
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: res[k] for k in ("total_ms", "spread_ms", "bf16_over_fp32", "classes")}))
    hip.close()


if __name__ == "__main__":
    main()
