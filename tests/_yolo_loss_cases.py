"""The inputs of tests/test_gpu_yolo_loss.py: one yolo layer's activated
output and truth boxes per case, built so that a named branch of the loss
runs.  tests/test_yolo_loss.py proves on the CPU, from the oracle's counters
alone, that every case reaches the branches in its ``needs``.

Predictions are built from the truths plus noise: the cell and anchor a truth
is responsible for gets that truth's box (IoU around 0.9, above ignore_thresh
0.5 and truth_thresh 0.7), with class scores above 0.25 for every other truth
and below it for the rest; all other cells hold class scores below 0.25.
"""
import functools
import math

import numpy as np

from _yolo_loss_oracle import yolo_loss

F = np.float32

ANCHORS6 = (10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319)                       # yolov3-tiny
ANCHORS9 = (10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326)  # yolov3

# a truth: (x, y, anchor whose shape it takes, class, scale of that shape);
# "end": a terminator row (x == 0) before max rows are used
CASES = {
    # h != w, the list completely full (no terminator row), two images' worth
    # of branches in one: matched and unmatched cells over ignore_thresh
    "3x5_full_list": dict(
        h=3, w=5, classes=3, total=6, mask=(0, 1, 2), batch=1, max_boxes=4,
        truths=[[(0.13, 0.2, 0, 0, 1.0), (0.5, 0.5, 1, 1, 1.1), (0.9, 0.8, 2, 2, 0.9),
                 (0.3, 0.7, 1, 0, 1.0)]],
        needs=("truth_writes", "ignored", "unmatched")),
    # batch 3: an empty list, a list ending early with a negative class in
    # the middle, a full list with a class >= classes in the middle and a
    # truth whose best anchor (0) lies outside the mask
    "3x5_lists": dict(
        h=3, w=5, classes=3, total=6, mask=(3, 4, 5), batch=3, max_boxes=4,
        truths=[[],
                [(0.3, 0.3, 3, 1, 1.0), (0.6, 0.6, 4, -1, 1.0), (0.7, 0.2, 4, 2, 1.0), "end"],
                [(0.5, 0.5, 5, 0, 0.8), (0.2, 0.8, 3, 3, 1.0), (0.85, 0.4, 0, 1, 1.0),
                 (0.1, 0.1, 4, 2, 1.0)]],
        needs=("truth_writes", "invalid_class", "outside_mask", "ignored")),
    # 13x13, three images, max=200 with lists ending early, two truths of one
    # class in the same cell with the same best anchor
    "13x13_same_cell": dict(
        h=13, w=13, classes=3, total=9, mask=(6, 7, 8), batch=3, max_boxes=200,
        truths=[[(0.52, 0.52, 7, 1, 1.0), (0.53, 0.51, 7, 1, 1.05), (0.2, 0.3, 6, 0, 1.0), "end"],
                [(0.8, 0.8, 8, 2, 0.7), (0.1, 0.9, 2, 0, 1.0), "end"],
                ["end"]],
        needs=("truth_writes", "rewritten", "ignored", "unmatched", "outside_mask")),
    # 80 classes: more than one wave of class lanes; the same cell hit twice
    # with different classes
    "2x3_classes80": dict(
        h=2, w=3, classes=80, total=6, mask=(0, 1, 2), batch=1, max_boxes=200,
        truths=[[(0.5, 0.3, 1, 17, 1.0), (0.52, 0.32, 1, 71, 1.0), (0.9, 0.9, 2, 79, 1.0),
                 "end"]],
        needs=("truth_writes", "rewritten")),
    # 17x17 = 289 cells: two workgroups of the cell pass per (image, anchor),
    # with a responsible cell in the second one (cell 16*17 + 15)
    "17x17_two_blocks": dict(
        h=17, w=17, classes=3, total=6, mask=(0, 1, 2), batch=1, max_boxes=4,
        truths=[[(0.9, 0.97, 2, 1, 1.0), (0.1, 0.1, 1, 0, 1.0), "end"]],
        needs=("truth_writes", "ignored", "unmatched")),
    "13x13_truth_thresh": dict(
        h=13, w=13, classes=3, total=6, mask=(3, 4, 5), batch=1, max_boxes=4, truth_thresh=0.7,
        truths=[[(0.4, 0.4, 3, 0, 1.0), (0.7, 0.6, 4, 2, 1.0), "end"]],
        needs=("truth_thresh", "truth_writes", "rewritten")),
    "3x5_iou_thresh": dict(
        h=3, w=5, classes=3, total=6, mask=(3, 4, 5), batch=3, max_boxes=4, iou_thresh=0.2,
        truths=[[(0.5, 0.5, 4, 1, 1.0), (0.1, 0.8, 3, 0, 1.0), "end"],
                [(0.9, 0.2, 5, 2, 1.0), "end"], []],
        needs=("second_anchor", "averaged", "truth_writes")),
    # NaN and +Inf objectness in images that have truths (reset to 0) and a
    # +Inf in an image that has none (kept: its delta is -Inf, the cost +Inf)
    "13x13_nan_inf": dict(
        h=13, w=13, classes=3, total=6, mask=(0, 1, 2), batch=3, max_boxes=200,
        truths=[[(0.3, 0.6, 1, 1, 1.0), "end"], [(0.6, 0.3, 2, 0, 1.0), (0.2, 0.2, 0, 2, 1.0),
                                                  "end"], []],
        bad_obj=[(0, 0, 5, float("nan")), (0, 2, 100, float("inf")), (1, 1, 37, float("nan")),
                 (1, 0, 168, float("inf")), (2, 1, 9, float("inf"))],
        needs=("nan_reset", "truth_writes")),
}


def _net_size(c):
    return 32 * c["w"], 32 * c["h"]


def kwargs_of(name):
    c = CASES[name]
    anchors = ANCHORS6 if c["total"] == 6 else ANCHORS9
    net_w, net_h = _net_size(c)
    return dict(batch=c["batch"], n=len(c["mask"]), classes=c["classes"], h=c["h"], w=c["w"],
                total=c["total"], mask=c["mask"], biases=tuple(float(a) for a in anchors),
                max_boxes=c["max_boxes"], net_w=net_w, net_h=net_h,
                ignore_thresh=float(F(c.get("ignore_thresh", 0.5))),
                truth_thresh=float(F(c.get("truth_thresh", 1.0))),
                iou_thresh=float(F(c.get("iou_thresh", 1.0))),
                iou_normalizer=float(F(0.75)), obj_normalizer=float(F(1.0)))


@functools.lru_cache(maxsize=None)
def build(name):
    """(output [batch*outputs] float32, truth [batch, max*6] float32, kwargs)."""
    c, kw = CASES[name], kwargs_of(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    B, n, cl, h, w = kw["batch"], kw["n"], kw["classes"], kw["h"], kw["w"]
    hw = h * w
    out = np.empty((B, n, cl + 5, hw), dtype=F)
    out[:, :, 0:2] = rng.uniform(0.1, 0.9, (B, n, 2, hw))
    out[:, :, 2:4] = rng.normal(0, 0.3, (B, n, 2, hw))
    out[:, :, 4] = rng.uniform(0.05, 0.95, (B, n, hw))
    out[:, :, 5:] = rng.uniform(0.0, 0.2, (B, n, cl, hw))
    truth = np.zeros((B, kw["max_boxes"], 6), dtype=F)
    bias = kw["biases"]
    for b, rows in enumerate(c["truths"]):
        for t, row in enumerate(rows):
            if row == "end":
                break
            x, y, an, cls, s = row
            tw, th = s * bias[2 * an] / kw["net_w"], s * bias[2 * an + 1] / kw["net_h"]
            truth[b, t] = (x, y, tw, th, cls, t + 1)
            if an not in kw["mask"]:
                continue
            i, j, a = int(x * w), int(y * h), kw["mask"].index(an)
            cell = j * w + i
            fit = (x * w - i, y * h - j, math.log(s), math.log(s))
            out[b, a, 0:4, cell] = np.asarray(fit) + rng.normal(0, 0.02, 4)
            if t % 2 == 0:  # every other truth's cell holds class scores above 0.25
                out[b, a, 5:, cell] = rng.uniform(0.3, 0.9, cl)
        assert len(rows) <= kw["max_boxes"] + (1 if rows and rows[-1] == "end" else 0)
    for b, a, cell, v in c.get("bad_obj", ()):
        out[b, a, 4, cell] = v
    out.setflags(write=False)
    truth.setflags(write=False)
    return out.reshape(-1), truth.reshape(B, -1), kw


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's result for a case, computed once and shared."""
    out, truth, kw = build(name)
    return yolo_loss(out, truth, **kw)
