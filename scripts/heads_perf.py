#!/usr/bin/env python3
"""Launch time and byte rate of the dropout kernels: forward (separate
buffers and in place) and backward (in place, the layer's call) at N = 65 536
(deepCIFAR10's first dropout layer at batch 32), 2^20 and 2^26, each timed
alone with HIP events (warm-up launches, then the median of several windows
of repeated launches on the backend's stream).

Algorithmic bytes: 12 per element for every dropout call (forward: read src,
write rnd and dst; backward: read src and rnd, write dst).  As the in-repo
yardstick ``hip.copy`` (unit strides) is timed at the same N in the same
process: 8 bytes per element.  Buffers of 2^26 floats are 256 MiB each, the
size of the last-level cache, so that row is an HBM figure; the two small
rows stay in cache and mostly measure the launch.  One JSON line to stdout.

  python scripts/heads_perf.py > profiles/heads_perf.json
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tensorium_amd.nnhip import TNNHip  # noqa: E402


def timed(fn, reps=20, windows=7, warmup=3):
    """Median over ``windows`` of the mean launch time (ms) of ``reps``
    back-to-back launches."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[65536, 1 << 20, 1 << 26])
    ap.add_argument("--probability", type=float, default=0.2)
    a = ap.parse_args()
    hip = TNNHip(0)
    p, scale, seed = a.probability, 1.0 / (1.0 - a.probability), 1234567
    rows = []
    for n in a.sizes:
        src = torch.rand(n, device="cuda")
        rnd = torch.empty(n, device="cuda")
        dst = torch.empty(n, device="cuda")
        t = {
            "forward": (12, timed(lambda: hip.forwardDropout(n, src, p, scale, rnd, dst, seed))),
            "forward_in_place": (12, timed(lambda: hip.forwardDropout(n, dst, p, scale, rnd, dst,
                                                                       seed))),
            "backward_in_place": (12, timed(lambda: hip.backwardDropout(n, dst, p, scale, rnd,
                                                                         dst))),
            "copy": (8, timed(lambda: hip.copy(n, src, 0, 1, dst, 0, 1))),
        }
        row = {"N": n}
        for k, (by, ms) in t.items():
            row[k] = {"us": round(ms * 1e3, 2), "bytes_per_element": by,
                      "tbs": round(by * n / ms / 1e9, 3)}
        rows.append(row)
        del src, rnd, dst
    print(json.dumps({"device": torch.cuda.get_device_name(0), "probability": p, "rows": rows}))


if __name__ == "__main__":
    main()
