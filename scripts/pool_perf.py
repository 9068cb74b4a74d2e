#!/usr/bin/env python3
"""HBM rates of the pooling kernels on the six max pools of yolov3-tiny at
416 px, batch 8: forward with and without the int64 indexes, and backward,
each timed alone with HIP events (warm-up launches, then the median of several
windows of repeated launches on the kernel's stream).

Algorithmic bytes: 4 per input element and per output element, 8 per stored
index (forward without indexes: no index bytes; backward: state.delta counted
once, although it is read and, where named, written).  As the in-repo
yardstick, ``upSample`` forward (stride 2) is timed at the same byte count
(4 bytes per small and per large element).  With ``--ceiling FILE`` (the JSON
line of scripts/hbm_ceiling.py, taken in the same session) every rate is also
given as a fraction of that file's 1600 MiB read+write copy rate; tensors of
a few tens of MB stay in the 256 MiB last-level cache between launches, so
the file's 64 MiB figures are the fairer bound for the small layers.  One
JSON line to stdout.

  python scripts/hbm_ceiling.py > ceiling.json
  python scripts/pool_perf.py --ceiling ceiling.json
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tensorium_amd import darknet as dn  # noqa: E402
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--ceiling", help="JSON written by scripts/hbm_ceiling.py")
    a = ap.parse_args()
    ceiling = json.loads(Path(a.ceiling).read_text()) if a.ceiling else None
    hbm = ceiling["1600MiB"]["copy_r1w1"] if ceiling else None
    hip = TNNHip(0)
    B = a.batch
    net = dn.Network(dn.parse_cfg(dn.yolov3_tiny_cfg(a.size, batch=B)))
    rows = []
    for l in (l for l in net.layers if l.kind == "maxpool"):
        nin, nout = B * l.c * l.h * l.w, B * l.out_size
        x = torch.rand(nin, device="cuda")
        out = torch.empty(nout, device="cuda")
        idx = torch.empty(nout, dtype=torch.int64, device="cuda")
        d = torch.rand(nout, device="cuda")
        sd = torch.zeros(nin, device="cuda")
        geo = (l.stride_x, l.stride_y, l.pad, l.size)
        by_idx, by_plain = 4 * (nin + nout) + 8 * nout, 4 * (nin + nout)
        row = {"layer": l.index,
               "shape": f"{l.c}x{l.h}x{l.w} k{l.size}s{l.stride_x}->{l.out_h}x{l.out_w}",
               "bytes_with_indexes": by_idx, "bytes_no_indexes": by_plain}
        t = {
            "forward_indexes": (by_idx, timed(lambda: hip.forwardMaxPool(
                B, l.out_c, l.out_h, l.out_w, x, l.c, l.h, l.w, *geo, idx, out))),
            "forward_no_indexes": (by_plain, timed(lambda: hip.forwardMaxPool(
                B, l.out_c, l.out_h, l.out_w, x, l.c, l.h, l.w, *geo, None, out))),
            "backward": (by_idx, timed(lambda: hip.backwardMaxPool(
                B, l.out_c, l.out_h, l.out_w, sd, idx, d, l.h, l.w, *geo))),
        }
        # upSample forward moving the same bytes: planes of the pooled size
        planes = max(1, round(by_idx / (20 * l.out_h * l.out_w)))
        small = torch.rand(planes * l.out_h * l.out_w, device="cuda")
        big = torch.empty(4 * small.numel(), device="cuda")
        t["upsample_same_bytes"] = (20 * small.numel(), timed(lambda: hip.upSample(
            1, planes, l.out_h, l.out_w, small, 2, 1, 1.0, big)))
        for k, (by, ms) in t.items():
            row[k] = {"us": round(ms * 1e3, 2), "gbs": round(by / ms / 1e6, 1)}
            if hbm:
                row[k]["of_hbm_copy"] = round(by / ms / 1e6 / hbm, 3)
        rows.append(row)
        del x, out, idx, d, sd, small, big
    print(json.dumps({"batch": B, "size": a.size, "device": torch.cuda.get_device_name(0),
                      "hbm_copy_1600MiB_gbs": hbm, "ceiling": ceiling, "pools": rows}))


if __name__ == "__main__":
    main()
