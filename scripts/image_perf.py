#!/usr/bin/env python3
"""Image preprocessing on the device against the copies around it: batch 8 of
1920x1080 and of 640x480 decoded RGB bytes -> 416x416 net input, resize and
letterbox (``TNNHip.imageToInput``).

Per source size and mode: the kernel's time; beside it ``hip.copy`` of as many
floats as the kernel writes (the floor of writing dst), the host->device copy
of the batch*3*416*416 floats a host-side resize would send (from pinned and
from pageable memory), and the host->device copy of the source bytes the
device route sends instead (pinned and pageable).  Each figure: warm-up calls,
then the median over several windows of the mean of repeated calls between two
device events.  The achieved rate counts every source byte once plus every
dst byte over the kernel's time; the repeated calls find the source (50 MB at
1920x1080, 7 MB at 640x480) in the Infinity Cache, so it is a rate of bytes
moved, set against HBM's 8 TB/s only for scale.
Writes one JSON document (default profiles/image_perf.json) and prints it.

  python scripts/image_perf.py [--out FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tensorium_amd.nnhip import TNNHip  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, HBM3E specification


def timed(fn, reps=20, windows=7, warmup=3):
    """Median over ``windows`` of the mean time (ms) of ``reps`` back-to-back calls."""
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "image_perf.json"))
    a = ap.parse_args()
    hip = TNNHip(0)
    B, S = a.batch, a.size
    n_dst = B * 3 * S * S
    dst = torch.empty(n_dst, device="cuda")
    other = torch.empty(n_dst, device="cuda")
    host_pin = torch.rand(n_dst).pin_memory()
    host_page = torch.rand(n_dst)
    copy_ms = timed(lambda: hip.copy(n_dst, other, 0, 1, dst, 0, 1))
    floats_pinned_ms = timed(lambda: dst.copy_(host_pin, non_blocking=True), reps=5)
    floats_pageable_ms = timed(lambda: dst.copy_(host_page, non_blocking=True), reps=5)
    rows = []
    for w, h in ((1920, 1080), (640, 480)):
        rng = np.random.default_rng(w)
        src_host = torch.from_numpy(rng.integers(0, 256, B * h * w * 3, dtype=np.uint8))
        src_pin = src_host.pin_memory()
        src = src_host.cuda()
        geom = [(b * h * w * 3, w, h, w * 3) for b in range(B)]
        bytes_pinned_ms = timed(lambda: src.copy_(src_pin, non_blocking=True), reps=5)
        bytes_pageable_ms = timed(lambda: src.copy_(src_host, non_blocking=True), reps=5)
        for letter in (False, True):
            placed = hip.imageToInput(src, geom, 3, S, S, dst, letter=letter)
            ms = timed(lambda: hip.imageToInput(src, geom, 3, S, S, dst, letter=letter))
            moved = src.numel() + 4 * n_dst
            costs = {"kernel": ms, "source_bytes_from_pinned": bytes_pinned_ms,
                     "dst_write_floor_copy": copy_ms}
            rows.append({
                "source": [w, h], "mode": "letterbox" if letter else "resize",
                "placed": list(placed[0]),
                "kernel_ms": round(ms, 4),
                "copy_of_dst_floats_ms": round(copy_ms, 4),
                "source_bytes": src.numel(), "dst_bytes": 4 * n_dst,
                "source_bytes_h2d_pinned_ms": round(bytes_pinned_ms, 4),
                "source_bytes_h2d_pageable_ms": round(bytes_pageable_ms, 4),
                "dst_floats_h2d_pinned_ms": round(floats_pinned_ms, 4),
                "dst_floats_h2d_pageable_ms": round(floats_pageable_ms, 4),
                "bytes_moved_per_s": round(moved / (ms * 1e-3)),
                "fraction_of_hbm_peak": round(moved / (ms * 1e-3) / HBM_PEAK, 4),
                "largest_cost": max(costs, key=costs.get)})
    doc = {"batch": B, "net": [S, S], "channels": 3, "device": torch.cuda.get_device_name(0),
           "hbm_peak_bytes_per_s": HBM_PEAK, "cases": rows}
    text = json.dumps(doc, indent=1)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
