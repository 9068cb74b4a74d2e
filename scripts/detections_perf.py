#!/usr/bin/env python3
"""Detections on the device against the copy they remove: the three YOLOv3
heads at batch 8 / 416 px (13^2, 26^2, 52^2; 80 classes) on synthetic activated
outputs, at two densities: about 100 and about 2000 of an image's 10647
candidates above thresh 0.25.

Per density: the time of collect (the counter reset and ``yoloDetections``
over the three heads), of collect + ``nmsSort`` at 0.45 (NMS works in place,
so it is timed behind the collect that rebuilds its rows; its own time is the
difference), and of bringing the counters and the used rows back.  Beside
them the plain device->host copy of the three yolo outputs, to pinned and to
pageable host memory: the floor of any host route, and what the device path
replaces.  Each device figure: warm-up calls, then the median over several
windows of the mean of repeated calls between two device events; the rows'
copy back, which synchronises, by the host clock.
Writes one JSON document (default profiles/detections_perf.json) and prints it.

  python scripts/detections_perf.py [--out FILE]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tensorium_amd import darknet as dn  # noqa: E402
from tensorium_amd.nnhip import TNNHip  # noqa: E402

THRESH, NMS = 0.25, 0.45


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


def host_timed(fn, reps=10, windows=7, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / reps)
    return statistics.median(ms)


def make_output(rng, l, batch, share):
    """Activated outputs of one head: ``share`` of the candidates with an
    objectness in (0.25, 1), the rest below; one class of each candidate in
    (0.5, 1), the others in (0, 0.3)."""
    hw = l.h * l.w
    o = rng.uniform(0.02, 0.98, (batch, l.anchors, l.classes + 5, hw)).astype(np.float32)
    o[:, :, 2:4] = rng.normal(0, 0.5, (batch, l.anchors, 2, hw))
    above = rng.random((batch, l.anchors, hw)) < share
    obj = np.where(above, rng.uniform(0.26, 1.0, above.shape), rng.uniform(0.0, 0.24, above.shape))
    o[:, :, 4] = obj
    o[:, :, 5:] = rng.uniform(0.0, 0.3, (batch, l.anchors, l.classes, hw))
    hot = rng.integers(0, l.classes, (batch, l.anchors, hw))
    bi, ai, ci = np.meshgrid(np.arange(batch), np.arange(l.anchors), np.arange(hw), indexing="ij")
    o[bi, ai, 5 + hot, ci] = rng.uniform(0.5, 1.0, hot.shape)
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "detections_perf.json"))
    a = ap.parse_args()
    hip = TNNHip(0)
    B = a.batch
    net = dn.Network(dn.parse_cfg(dn.yolov3_cfg(a.size, batch=B)))
    ys = [l for l in net.layers if l.kind == "yolo"]
    classes = ys[0].classes
    cap = sum(l.anchors * l.h * l.w for l in ys)
    floats = sum(B * l.out_size for l in ys)
    counts = torch.zeros(B, dtype=torch.int64, device="cuda")
    boxes = torch.empty(B * cap * 4, device="cuda")
    obj = torch.empty(B * cap, device="cuda")
    probs = torch.empty(B * cap * classes, device="cuda")
    pin = {l.index: torch.empty(B * l.out_size).pin_memory() for l in ys}
    page = {l.index: torch.empty(B * l.out_size) for l in ys}
    rows, pinned = [], {}
    for target in (100, 2000):
        rng = np.random.default_rng(target)
        outs = {l.index: torch.from_numpy(make_output(rng, l, B, target / cap).reshape(-1)).cuda()
                for l in ys}

        def collect():
            hip.fill(2 * B, counts.data_ptr(), 0, 0.0, 1)
            for l in ys:
                hip.yoloDetections(B, l.anchors, classes, l.h, l.w, l.total, l.mask, l.biases,
                                   net.w, net.h, 640, 480, THRESH, False, True, outs[l.index], cap,
                                   counts, boxes, obj, probs)

        def collect_nms():
            collect()
            hip.nmsSort(B, cap, classes, counts, boxes, obj, probs, NMS)

        def rows_back():  # what HipDarknet.detections does after the kernels
            pinned["rows"] = dn.detection_rows_to_host(torch, counts.cpu().tolist(), cap, classes,
                                                       boxes, obj, probs, pinned.get("rows"))[1]

        def outputs_to(host):
            for l in ys:
                host[l.index].copy_(outs[l.index], non_blocking=True)

        collect_ms = timed(collect)
        both_ms = timed(collect_nms)
        hip.finish()
        taken = counts.cpu().tolist()
        view = probs.reshape(B, cap, classes)
        scores = sum(int((view[b, :n] != 0).sum().item()) for b, n in enumerate(taken))
        per_class = max(int((view[b, :n] != 0).sum(dim=0).max().item()) for b, n in enumerate(taken))
        back_ms = host_timed(rows_back)
        pinned_ms = timed(lambda: outputs_to(pin), reps=5)
        pageable_ms = timed(lambda: outputs_to(page), reps=5)
        stages = {"collect": collect_ms, "nms": both_ms - collect_ms, "rows_back": back_ms}
        rows.append({"target_rows_per_image": target,
                     "rows_per_image": taken,
                     "nonzero_scores_after_nms": scores,
                     "most_nonzero_scores_in_one_class_after_nms": per_class,
                     "collect_ms": round(collect_ms, 4),
                     "collect_nms_ms": round(both_ms, 4),
                     "nms_ms": round(both_ms - collect_ms, 4),
                     "rows_back_host_clock_ms": round(back_ms, 4),
                     "outputs_to_pinned_ms": round(pinned_ms, 4),
                     "outputs_to_pageable_ms": round(pageable_ms, 4),
                     "device_route_ms": round(both_ms + back_ms, 4),
                     "device_route_under_pinned_copy": both_ms + back_ms < pinned_ms,
                     "slowest_stage": max(stages, key=stages.get)})
    doc = {"batch": B, "size": a.size, "classes": classes, "capacity": cap,
           "thresh": THRESH, "nms": NMS, "device": torch.cuda.get_device_name(0),
           "yolo_output_floats": floats, "densities": rows}
    text = json.dumps(doc, indent=1)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
