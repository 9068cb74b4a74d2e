#!/usr/bin/env python3
"""Launch times of the global average pool kernels on the planes classifiers
have at batch 64: darknet19 at 256 px (64*1000 planes of 64), darknet53 at
256 px (64*1024 of 64) and at 416 px (64*1024 of 169), and 64*2048 planes of
49.  Forward and backward, and as the forward's baseline the batch-norm
``means(srcSize, dstSize=planes, groups=1)`` on the same buffers, which
computes the same quotients (0 + vssum, divided by n) with one thread a plane.

Method: HIP events around a window of back-to-back launches on the backend's
stream, after a warm-up; the launch count is calibrated so that a window lasts
at least half a second.  Every launch takes the next of a ring of input
buffers that together exceed 512 MiB, twice the last-level cache, so the
input comes from HBM.  The new forward and the baseline alternate window by
window, and every window is run twice: both values are reported, their
difference is the run-to-run spread.  ``us`` is the time between launches in
a full queue, so it holds the launch gap as well as the kernel.  ``host_us``
is the host's time a launch in the same window; once the queue is full the
host waits for the device, so it follows ``us`` and bounds nothing by itself.
Its smallest value in a run is an upper bound on what one enqueue costs the
host: a ``us`` near that value may be the enqueue rate, not the kernel.

Reported per kernel: us a launch (both runs), algorithmic bytes (forward: 4
per input element and per output; backward: state.delta read and written, 8
per element, plus 4 per delta), GB/s of those bytes at the better run, and
that rate over the rate of a 1600 MiB ``copy`` (read + write) timed in the
same process.  One JSON document, to --out.

  python scripts/global_avgpool_perf.py --out profiles/global_avgpool_perf.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tensorium_amd.nnhip import TNNHip  # noqa: E402

SHAPES = [("darknet19 256px", 64 * 1000, 64), ("darknet53 256px", 64 * 1024, 64),
          ("darknet53 416px", 64 * 1024, 169), ("2048 channels 7x7", 64 * 2048, 49)]
RING_BYTES = 512 << 20


def window(fns, reps):
    """(device us, host us) a launch of ``reps`` launches, fns taken in turn."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for i in range(reps):
        fns[i % len(fns)]()
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, host * 1e6 / reps


def calibrate(fns, seconds):
    for f in fns:   # warm-up: every buffer of the ring once
        f()
    us, _ = window(fns, 200)
    return max(200, int(seconds * 1e6 / us) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/global_avgpool_perf.json")
    ap.add_argument("--seconds", type=float, default=0.5, help="least length of a window")
    a = ap.parse_args()
    hip = TNNHip(0)
    n = 1600 * 1024 * 1024 // 4
    x, y = torch.rand(n, device="cuda"), torch.empty(n, device="cuda")
    copy = [lambda: hip.copy(n, x, 0, 1, y, 0, 1)]
    reps = calibrate(copy, a.seconds)
    copy_us = min(window(copy, reps)[0] for _ in range(2))
    hbm = 2 * n * 4 / copy_us / 1e3   # GB/s
    del x, y
    rows = []
    for name, planes, plane in SHAPES:
        total = planes * plane
        ring = RING_BYTES // (4 * total) + 1
        xs = [torch.randn(total, device="cuda") for _ in range(ring)]
        out = torch.empty(planes, device="cuda")
        d = torch.randn(planes, device="cuda")
        kernels = {
            "forward": ([lambda x=x: hip.forwardGlobalAvgPool(planes, 1, plane, 1, x, out)
                         for x in xs], 4 * (total + planes)),
            "means_baseline": ([lambda x=x: hip.means(total, planes, 1, x, 0, out) for x in xs],
                               4 * (total + planes)),
            # (the ring's buffers serve as state.delta: the values grow, the time does not)
            "backward": ([lambda x=x: hip.backwardGlobalAvgPool(planes, 1, plane, 1, d, x)
                          for x in xs], 8 * total + 4 * planes),
        }
        reps = {k: calibrate(f, a.seconds) for k, (f, _) in kernels.items()}
        runs = {k: [] for k in kernels}
        for _ in range(2):   # forward and baseline alternate; then the repeat
            for k, (f, _) in kernels.items():
                runs[k].append(window(f, reps[k]))
        row = {"shape": name, "planes": planes, "n": plane, "ring_buffers": ring}
        for k, (_, by) in kernels.items():
            us = [r[0] for r in runs[k]]
            row[k] = {"us": [round(u, 2) for u in us],
                      "host_us": [round(r[1], 2) for r in runs[k]], "launches": reps[k],
                      "bytes": by, "gbs": round(by / min(us) / 1e3, 1),
                      "of_hbm_copy": round(by / min(us) / 1e3 / hbm, 3)}
        f, b = row["forward"]["us"], row["means_baseline"]["us"]
        row["forward_over_baseline"] = round(min(f) / min(b), 3)
        row["spread"] = round(max(abs(f[0] - f[1]) / min(f), abs(b[0] - b[1]) / min(b)), 3)
        rows.append(row)
        del xs, out, d, kernels
    doc = {"device": torch.cuda.get_device_name(0), "window_seconds": a.seconds,
           "hbm_copy_1600MiB_gbs": round(hbm, 1), "shapes": rows}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
