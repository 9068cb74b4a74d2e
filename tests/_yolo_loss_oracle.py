"""Per-element restatement of TYoloLayer.forward under state.isTraining
(nyololayer.pas:835-1003 with processBatch 500-774, deltaBox 124-202,
deltaClass 204-251, averageDeltas 253-269, compareClass 272-281, getBox
105-122; box_iou ntypes.pas:1059-1108; sumSqr ntensors.pas:9333-9341), for
the settings the device loss builds: iou_loss=mse, iou_thresh_kind=iou,
scale_x_y=1, no focal_loss / objectness_smooth / label_smooth_eps /
new_coords / counters_per_class / map / embedding_layer, [net] without
adversarial and bad-label rejection.

Written from the reference's expressions with FPC's typing: every variable
is a ``single`` (np.float32, each operation rounded), except where exp or ln
enters an expression; those return a real, so the rest of that expression is
evaluated in float64 and rounded once on the assignment.

Besides the results it counts how often each branch ran, so that a test can
prove from the oracle alone that its inputs reach the branch it was built
for.  One departure, shared with the device code: a truth whose cell
trunc(x*w), trunc(y*h) lies outside the grid is skipped in the truth pass
(the reference indexes it unchecked); ``out_of_grid`` counts those.
"""
import math

import numpy as np

F = np.float32
D = np.float64

COUNTERS = ("ignored", "truth_thresh", "truth_writes", "rewritten", "second_anchor", "averaged",
            "invalid_class", "outside_mask", "nan_reset")


def overlap(x1, w1, x2, w2):
    l1 = F(x1 - F(w1 / F(2)))
    l2 = F(x2 - F(w2 / F(2)))
    left = l1 if l1 > l2 else l2
    r1 = F(x1 + F(w1 / F(2)))
    r2 = F(x2 + F(w2 / F(2)))
    right = r1 if r1 < r2 else r2
    return F(right - left)


def box_intersection(a, b):
    w = overlap(a[0], a[2], b[0], b[2])
    h = overlap(a[1], a[3], b[1], b[3])
    if w < 0 or h < 0:
        return F(0)
    return F(w * h)


def box_iou(a, b):
    i = box_intersection(a, b)
    u = F(F(F(a[2] * a[3]) + F(b[2] * b[3])) - i)
    if i == 0 or u == 0:
        return F(0)
    return F(i / u)


def _trunc(v):
    return int(math.trunc(float(v)))


def _bad(v):
    return bool(np.isnan(v) or np.isinf(v))


class _Layer:
    def __init__(self, out, truth, batch, n, classes, h, w, total, mask, biases, max_boxes, net_w,
                 net_h, ignore_thresh, truth_thresh, iou_thresh, iou_normalizer, obj_normalizer):
        self.batch, self.n, self.classes, self.h, self.w = batch, n, classes, h, w
        self.total, self.mask, self.max_boxes = total, [int(m) for m in mask], max_boxes
        self.biases = [F(v) for v in biases]
        self.net_w, self.net_h = net_w, net_h
        self.ignore_thresh, self.truth_thresh = F(ignore_thresh), F(truth_thresh)
        self.iou_thresh = F(iou_thresh)
        self.iou_normalizer, self.obj_normalizer = F(iou_normalizer), F(obj_normalizer)
        self.outputs = n * (classes + 5) * h * w
        self.output = np.array(out, dtype=F).reshape(-1).copy()
        assert self.output.size == batch * self.outputs
        self.truth = np.array(truth, dtype=F).reshape(-1)
        assert self.truth.size == batch * max_boxes * 6
        self.delta = np.zeros(batch * self.outputs, dtype=F)  # delta.fill(0)
        self.total_bbox = 0
        self.rewritten_bbox = 0
        self.count = [0] * batch
        self.tot_iou = [F(0)] * batch
        self.c = dict.fromkeys(COUNTERS + ("unmatched", "out_of_grid"), 0)

    def entry_index(self, b, location, entry):
        wh = self.w * self.h
        n_, loc = divmod(location, wh)
        return b * self.outputs + n_ * (self.classes + 5) * wh + entry * wh + loc

    def truth_box(self, b, t):
        o = t * 6 + b * self.max_boxes * 6
        return tuple(self.truth[o:o + 4])

    def get_box(self, an, index, col, row, stride):
        o = self.output
        x = F(F(F(col) + o[index]) / F(self.w))
        y = F(F(F(row) + o[index + stride]) / F(self.h))
        w = F(np.exp(D(o[index + 2 * stride])) * D(self.biases[2 * an]) / D(self.net_w))
        h = F(np.exp(D(o[index + 3 * stride])) * D(self.biases[2 * an + 1]) / D(self.net_h))
        return (x, y, w, h)

    def delta_box(self, truth, an, index, i, j, stride):
        o, d = self.output, self.delta
        scale = F(F(2) - F(truth[2] * truth[3]))
        if any(d[index + k * stride] != 0 for k in range(4)):
            self.rewritten_bbox += 1
            self.c["rewritten"] += 1
        pred = self.get_box(an, index, i, j, stride)
        iou = box_iou(pred, truth)
        tx = F(F(truth[0] * F(self.w)) - F(i))
        ty = F(F(truth[1] * F(self.h)) - F(j))
        tw = F(np.log(D(F(F(truth[2] * F(self.w)) / self.biases[2 * an]))))
        th = F(np.log(D(F(F(truth[3] * F(self.h)) / self.biases[2 * an + 1]))))
        for k, t in enumerate((tx, ty, tw, th)):
            p = index + k * stride
            d[p] = F(d[p] + F(F(scale * F(t - o[p])) * self.iou_normalizer))
        return iou

    def delta_class(self, index, class_id, stride):
        o, d = self.output, self.delta
        p = index + stride * class_id
        if d[p] != 0:
            r = F(F(1) - o[p])
            if not _bad(r):
                d[p] = r
            return
        for n_ in range(self.classes):
            p = index + stride * n_
            r = F(F(1 if n_ == class_id else 0) - o[p])
            if not _bad(r):
                d[p] = r

    def compare_class(self, class_index, stride, thresh):
        return any(self.output[class_index + stride * j] > thresh for j in range(self.classes))

    def class_of(self, b, t):
        v = self.truth[t * 6 + b * self.max_boxes * 6 + 4]
        return _trunc(v) if np.isfinite(v) else None  # (trunc of NaN / Inf: no class)

    def process_batch(self, b):
        o, d, c = self.output, self.delta, self.c
        stride = self.w * self.h
        for j in range(self.h):
            for i in range(self.w):
                for n_ in range(self.n):
                    loc = n_ * stride + j * self.w + i
                    class_index = self.entry_index(b, loc, 5)
                    obj_index = self.entry_index(b, loc, 4)
                    box_index = self.entry_index(b, loc, 0)
                    pred = self.get_box(self.mask[n_], box_index, i, j, stride)
                    best_match_iou, best_iou, best_t = F(0), F(0), 0
                    for t in range(self.max_boxes):
                        truth = self.truth_box(b, t)
                        if truth[0] == 0:
                            break
                        class_id = self.class_of(b, t)
                        if class_id is None or class_id >= self.classes or class_id < 0:
                            continue
                        if _bad(o[obj_index]):
                            o[obj_index] = F(0)
                            c["nan_reset"] += 1
                        class_id_match = self.compare_class(class_index, stride, F(0.25))
                        iou = box_iou(pred, truth)
                        if iou > best_match_iou and class_id_match:
                            best_match_iou = iou
                        if iou > best_iou:
                            best_iou, best_t = iou, t
                    d[obj_index] = F(self.obj_normalizer * F(-o[obj_index]))
                    if best_match_iou > self.ignore_thresh:
                        d[obj_index] = F(0)
                        c["ignored"] += 1
                    elif best_iou > self.ignore_thresh:
                        c["unmatched"] += 1  # over the threshold, no class above 0.25
                    if best_iou > self.truth_thresh:
                        class_id = self.class_of(b, best_t)
                        if class_id is None or not 0 <= class_id < self.classes:
                            continue  # (row 0 taken with no overlap: not built, see the kernel)
                        d[obj_index] = F(self.obj_normalizer * F(F(1) - o[obj_index]))
                        self.delta_class(class_index, class_id, stride)
                        truth = self.truth_box(b, best_t)
                        self.delta_box(truth, self.mask[n_], box_index, i, j, stride)
                        self.total_bbox += 1
                        c["truth_thresh"] += 1
        for t in range(self.max_boxes):
            truth = self.truth_box(b, t)
            if truth[0] == 0:
                break
            class_id = self.class_of(b, t)
            if class_id is None or class_id >= self.classes or class_id < 0:
                c["invalid_class"] += 1
                continue
            fi, fj = F(truth[0] * F(self.w)), F(truth[1] * F(self.h))
            if not (np.isfinite(fi) and np.isfinite(fj)) or not (
                    0 <= _trunc(fi) < self.w and 0 <= _trunc(fj) < self.h):
                c["out_of_grid"] += 1
                continue
            i, j = _trunc(fi), _trunc(fj)
            shift = (F(0), F(0), truth[2], truth[3])
            best_iou, best_n = F(0), 0
            for n_ in range(self.total):
                pred = (F(0), F(0), F(self.biases[2 * n_] / F(self.net_w)),
                        F(self.biases[2 * n_ + 1] / F(self.net_h)))
                iou = box_iou(pred, shift)
                if iou > best_iou:
                    best_iou, best_n = iou, n_
            mask_n = self.mask.index(best_n) if best_n in self.mask else -1
            if mask_n >= 0:
                self.truth_write(b, mask_n, best_n, i, j, truth, class_id, stride)
                c["truth_writes"] += 1
            else:
                c["outside_mask"] += 1
            for n_ in range(self.total):
                mask_n = self.mask.index(n_) if n_ in self.mask else -1
                if mask_n >= 0 and n_ != best_n and self.iou_thresh < F(1.0):
                    pred = (F(0), F(0), F(self.biases[2 * n_] / F(self.net_w)),
                            F(self.biases[2 * n_ + 1] / F(self.net_h)))
                    if box_iou(pred, shift) > self.iou_thresh:
                        self.truth_write(b, mask_n, n_, i, j, truth, class_id, stride)
                        c["second_anchor"] += 1
        if self.iou_thresh < F(1.0):
            for j in range(self.h):
                for i in range(self.w):
                    for n_ in range(self.n):
                        loc = n_ * stride + j * self.w + i
                        if d[self.entry_index(b, loc, 4)] != 0:
                            self.average_deltas(self.entry_index(b, loc, 5),
                                                self.entry_index(b, loc, 0), stride)

    def truth_write(self, b, mask_n, an, i, j, truth, class_id, stride):
        o, d = self.output, self.delta
        loc = mask_n * stride + j * self.w + i
        iou = self.delta_box(truth, an, self.entry_index(b, loc, 0), i, j, stride)
        self.total_bbox += 1
        self.tot_iou[b] = F(self.tot_iou[b] + iou)
        obj_index = self.entry_index(b, loc, 4)
        d[obj_index] = F(F(F(1.0) * self.obj_normalizer) * F(F(1) - o[obj_index]))
        self.delta_class(self.entry_index(b, loc, 5), class_id, stride)
        self.count[b] += 1

    def average_deltas(self, class_index, box_index, stride):
        d = self.delta
        in_box = sum(1 for k in range(self.classes) if d[class_index + stride * k] > 0)
        if in_box > 0:
            for k in range(4):
                d[box_index + k * stride] = F(d[box_index + k * stride] / F(in_box))
            self.c["averaged"] += 1


def sum_sqr(x):
    """TTensor<T>.sumSqr: Result := Result + src[i]*src[i], ascending."""
    s = F(0)
    for v in np.asarray(x, dtype=F).reshape(-1):
        s = F(s + F(v * v))
    return s


def yolo_loss(out, truth, **kw):
    """The training forward of one yolo layer.  Keywords: batch, n, classes,
    h, w, total, mask, biases, max_boxes, net_w, net_h, ignore_thresh,
    truth_thresh, iou_thresh, iou_normalizer, obj_normalizer.  Returns a dict:
    delta, cost (float32), output (after the NaN reset), stats ([batch, 2]
    float32: count, tot_iou), total_bbox, rewritten_bbox, counters."""
    with np.errstate(all="ignore"):
        lay = _Layer(out, truth, **kw)
        for b in range(lay.batch):
            lay.process_batch(b)
        cost = sum_sqr(lay.delta)
    stats = np.array([[F(lay.count[b]), lay.tot_iou[b]] for b in range(lay.batch)], dtype=F)
    return dict(delta=lay.delta, cost=cost, output=lay.output, stats=stats.reshape(lay.batch, 2),
                total_bbox=lay.total_bbox, rewritten_bbox=lay.rewritten_bbox, counters=lay.c)


def layer_kwargs(l, net):
    """yolo_loss's keywords from a planned [yolo] Layer and its Network."""
    return dict(batch=net.batch, n=l.anchors, classes=l.classes, h=l.h, w=l.w, total=l.total,
                mask=l.mask, biases=l.biases, max_boxes=l.max_boxes, net_w=net.w, net_h=net.h,
                ignore_thresh=l.ignore_thresh, truth_thresh=l.truth_thresh,
                iou_thresh=l.iou_thresh, iou_normalizer=l.iou_normalizer,
                obj_normalizer=l.obj_normalizer)
