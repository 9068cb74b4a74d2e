#!/usr/bin/env python3
"""The device yolo loss against the copies it removes: the three YOLOv3 heads
at batch 8 / 416 px (13^2, 26^2, 52^2; 80 classes; max=200) with 1, 20 and 200
truths per image.

Per truth count: the time of the ``yoloLoss`` call per layer and summed, and
the time of what the reference's route moves before its CPU loop starts: the
device->host copy of the three outputs plus the host->device copy of the three
deltas, from and to pinned host memory (the faster, so the harder yardstick)
and pageable host memory.  Each figure: warm-up calls, then the median over
several windows of the mean of repeated calls between two device events.
Writes one JSON document (default profiles/yolo_loss_perf.json) and prints it.

  python scripts/yolo_loss_perf.py [--out FILE]
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
from tensorium_amd import darknet as dn  # noqa: E402
from tensorium_amd.nnhip import TNNHip  # noqa: E402


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


def make_truth(rng, net, layer, batch, count):
    """count boxes per image, each the shape of a random anchor (x0.7..1.4)."""
    t = np.zeros((batch, layer.max_boxes, 6), dtype=np.float32)
    an = rng.integers(0, layer.total, (batch, count))
    s = rng.uniform(0.7, 1.4, (batch, count))
    b = np.asarray(layer.biases, dtype=np.float64).reshape(-1, 2)
    t[:, :count, 0:2] = rng.uniform(0.02, 0.98, (batch, count, 2))
    t[:, :count, 2] = np.minimum(s * b[an, 0] / net.w, 0.99)
    t[:, :count, 3] = np.minimum(s * b[an, 1] / net.h, 0.99)
    t[:, :count, 4] = rng.integers(0, layer.classes, (batch, count))
    return t.reshape(batch, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "yolo_loss_perf.json"))
    a = ap.parse_args()
    hip = TNNHip(0)
    B = a.batch
    net = dn.Network(dn.parse_cfg(dn.yolov3_cfg(a.size, batch=B)))
    ys = [l for l in net.layers if l.kind == "yolo"]
    rng = np.random.default_rng(11)
    bufs = {}
    for l in ys:
        n = B * l.out_size
        o = rng.uniform(0.02, 0.98, (B, l.anchors, l.classes + 5, l.h * l.w)).astype(np.float32)
        o[:, :, 2:4] = rng.normal(0, 0.5, (B, l.anchors, 2, l.h * l.w))
        bufs[l.index] = dict(out=torch.from_numpy(o.reshape(-1)).cuda(),
                             delta=torch.zeros(n, device="cuda"),
                             cost=torch.zeros(1, device="cuda"),
                             stats=torch.zeros(2 * B, device="cuda"),
                             pin=torch.empty(n).pin_memory(), page=torch.empty(n))
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")

    def loss(l, truth):
        d = bufs[l.index]
        hip.yoloLoss(B, l.anchors, l.classes, l.h, l.w, l.total, l.mask, l.biases, l.max_boxes,
                     net.w, net.h, l.ignore_thresh, l.truth_thresh, l.iou_thresh,
                     l.iou_normalizer, l.obj_normalizer, d["out"], truth, d["delta"], d["cost"],
                     d["stats"], counters)

    def round_trip(host):
        for l in ys:
            d = bufs[l.index]
            d[host].copy_(d["out"], non_blocking=True)
        for l in ys:
            d = bufs[l.index]
            d["delta"].copy_(d[host], non_blocking=True)

    floats = sum(B * l.out_size for l in ys)
    copies = {"floats_each_way": floats,
              "pinned_ms": round(timed(lambda: round_trip("pin"), reps=5), 4),
              "pageable_ms": round(timed(lambda: round_trip("page"), reps=5), 4)}
    rows = []
    for count in (1, 20, 200):
        truth = torch.from_numpy(make_truth(rng, net, ys[0], B, count)).cuda()
        per = {}
        for l in ys:
            per[f"{l.h}x{l.w}"] = round(timed(lambda: loss(l, truth)), 4)
            nz = int((bufs[l.index]["delta"] != 0).sum().item())
            per[f"{l.h}x{l.w}_nonzero_deltas"] = nz
        total = round(timed(lambda: [loss(l, truth) for l in ys]), 4)
        rows.append({"truths_per_image": count, "yolo_loss_ms": per, "yolo_loss_sum_ms": total,
                     "under_pinned_round_trip": total < copies["pinned_ms"]})
    doc = {"batch": B, "size": a.size, "device": torch.cuda.get_device_name(0),
           "copy_round_trip": copies, "loss": rows}
    text = json.dumps(doc, indent=1)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
