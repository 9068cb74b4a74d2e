"""NumPy restatement of the reference's detection loops: TYoloLayer.
getDetectionCount / getDetections / correctBoxes (nyololayer.pas:378-498 with
getBox 105-122, not newCoords) and TDetections.doNMSSort with its Comparer
(ntypes.pas:1554-1565, 1612-1649; TBox.iou 1059-1108).

Written from the reference's expressions with FPC's typing: every variable is
a ``single`` (np.float32, each operation rounded), except that exp returns a
real, so its expression is evaluated in float64 and rounded once on the
assignment, and that integer / integer is a real.  The loops over candidates
and over later rows are NumPy array operations, one float32 operation per
Pascal operation; ``tests/test_detections.py`` holds them against the scalar
box_iou of tests/_yolo_loss_oracle.py.

Two documented departures, shared with the device code (include/tns.h): rows
keep their place through NMS, and equal non-zero scores order the lower row
first (the reference's QuickSort leaves their order unspecified).

Besides the results it counts what happened, so that a test can prove from
the oracle alone that its inputs reach what it was built for:
  taken         candidates that became rows
  nan           candidates dropped because their objectness is NaN
  zeroed_prob   objectness * class products not > thresh, written as 0
  suppressed    scores NMS turned from non-zero to 0
  chain         rows that a zeroed row overlapped above thresh and that end
                non-zero in that class (a row already zeroed suppresses nothing)
  ties          pairs of equal non-zero scores within one class
  near_thresh   IoUs NMS compared that lie within 1e-5 of its threshold
  zero_obj      zero-objectness rows, which NMS leaves out
"""
import numpy as np

F = np.float32
D = np.float64

COUNTERS = ("taken", "nan", "zeroed_prob", "suppressed", "chain", "ties", "near_thresh",
            "zero_obj")


def new_counters():
    return dict.fromkeys(COUNTERS, 0)


def _overlap(x1, w1, x2, w2):
    """overlap (ntypes.pas:1059-1075): one box (scalars) against many."""
    l1 = F(x1 - F(w1 / F(2)))
    l2 = x2 - w2 / F(2)
    left = np.where(l1 > l2, l1, l2)
    r1 = F(x1 + F(w1 / F(2)))
    r2 = x2 + w2 / F(2)
    right = np.where(r1 < r2, r1, r2)
    return right - left


def iou_many(a, boxes):
    """TBox.iou (ntypes.pas:1077-1108) of box ``a`` [4] with every row of
    ``boxes`` [m, 4], in singles."""
    boxes = np.asarray(boxes, dtype=F).reshape(-1, 4)
    a = np.asarray(a, dtype=F)
    with np.errstate(all="ignore"):
        w = _overlap(a[0], a[2], boxes[:, 0], boxes[:, 2])
        h = _overlap(a[1], a[3], boxes[:, 1], boxes[:, 3])
        inter = np.where((w < 0) | (h < 0), F(0), w * h).astype(F)
        union = (F(a[2] * a[3]) + boxes[:, 2] * boxes[:, 3]) - inter
        zero = (inter == 0) | (union == 0)
        q = inter / np.where(zero, F(1), union)
        res = np.where(zero, F(0), q).astype(F)
    assert w.dtype == F and union.dtype == F and q.dtype == F
    return res


def correct_boxes(boxes, im_w, im_h, net_w, net_h, relative, letter):
    """correctBoxes (nyololayer.pas:452-498) on rows [m, 4]; w, h there are
    the image's extents."""
    new_w, new_h = net_w, net_h
    if letter:
        if (net_w / im_w) < (net_h / im_h):       # integer / integer: reals
            new_h = (im_h * net_w) // im_w        # div
        else:
            new_w = (im_w * net_h) // im_h
    deltaw, deltah = F(net_w - new_w), F(net_h - new_h)
    with np.errstate(all="ignore"):
        ratiow, ratioh = F(D(new_w) / D(net_w)), F(D(new_h) / D(net_h))
        b = np.array(boxes, dtype=F).reshape(-1, 4)
        # (b.x - deltaw / 2.0 / netw) / ratiow, every step a single
        b[:, 0] = (b[:, 0] - F(F(deltaw / F(2)) / F(net_w))) / ratiow
        b[:, 1] = (b[:, 1] - F(F(deltah / F(2)) / F(net_h))) / ratioh
        b[:, 2] = b[:, 2] * F(F(1) / ratiow)
        b[:, 3] = b[:, 3] * F(F(1) / ratioh)
        if not relative:
            b[:, 0] = b[:, 0] * F(im_w)
            b[:, 2] = b[:, 2] * F(im_w)
            b[:, 1] = b[:, 1] * F(im_h)
            b[:, 3] = b[:, 3] * F(im_h)
    assert b.dtype == F
    return b


def get_detections(out, b, *, n, classes, h, w, mask, biases, net_w, net_h, im_w, im_h, thresh,
                   relative, letter, total=None, counters=None):
    """getDetectionCount + getDetections + correctBoxes (nyololayer.pas:
    378-498) for image ``b`` of one layer's output [batch][n][classes+5][h*w].
    Returns (boxes [m, 4], objectness [m], probs [m, classes]) in the
    reference's order: cell outer, anchor inner."""
    c = counters if counters is not None else new_counters()
    hw = h * w
    o = np.asarray(out, dtype=F).reshape(-1, n, classes + 5, hw)[b]
    o = np.transpose(o, (2, 0, 1)).reshape(hw * n, classes + 5)   # candidate = cell*n + anchor
    thresh = F(thresh)
    obj = o[:, 4]
    with np.errstate(all="ignore"):
        take = obj > thresh                       # strict; false for NaN (392-394, 424-426)
    c["nan"] += int(np.isnan(obj).sum())
    idx = np.flatnonzero(take)
    c["taken"] += idx.size
    cell, an = idx // n, idx % n
    row, col = cell // w, cell % w
    r = o[idx]
    bias = np.asarray([F(v) for v in biases], dtype=F)
    m = np.asarray(mask, dtype=np.int64)[an]
    boxes = np.empty((idx.size, 4), dtype=F)
    with np.errstate(all="ignore"):
        # getBox (105-122): (col + out) / w in singles; exp(out) * bias / netWidth
        # in reals, rounded on the assignment
        boxes[:, 0] = (col.astype(F) + r[:, 0]) / F(w)
        boxes[:, 1] = (row.astype(F) + r[:, 1]) / F(h)
        boxes[:, 2] = (np.exp(r[:, 2].astype(D)) * bias[2 * m].astype(D) / D(net_w)).astype(F)
        boxes[:, 3] = (np.exp(r[:, 3].astype(D)) * bias[2 * m + 1].astype(D) / D(net_h)).astype(F)
        prob = r[:, 4:5] * r[:, 5:]               # objectness * class_j, singles (438)
        keep = prob > thresh
    assert prob.dtype == F
    c["zeroed_prob"] += int((~keep).sum())
    probs = np.where(keep, prob, F(0)).astype(F)
    boxes = correct_boxes(boxes, im_w, im_h, net_w, net_h, relative, letter)
    return boxes, r[:, 4].copy(), probs


def order_of(scores, rows):
    """Comparer's order (ntypes.pas:1554-1565) over ``rows``: score
    descending; equal scores, the lower row first (the tie rule)."""
    return sorted(rows, key=lambda r: (-float(scores[r]), r))


def nms_sort(boxes, objectness, probs, thresh, counters=None, chains=True):
    """doNMSSort (ntypes.pas:1612-1649) on one image's rows; returns the new
    probs [m, classes], rows in place.  chains=False leaves the chain counter
    alone (it costs one IoU pass per zeroed row)."""
    c = counters if counters is not None else new_counters()
    boxes = np.asarray(boxes, dtype=F).reshape(-1, 4)
    objectness = np.asarray(objectness, dtype=F).reshape(-1)
    probs = np.array(probs, dtype=F).reshape(boxes.shape[0], -1)
    thresh = F(thresh)
    # the zero-objectness rows are swapped out of `total` (1619-1633)
    part = [r for r in range(boxes.shape[0]) if not objectness[r] == 0]
    c["zero_obj"] += boxes.shape[0] - len(part)
    for k in range(probs.shape[1]):
        s = probs[:, k]
        nz = [r for r in part if s[r] != 0]
        vals = np.array([s[r] for r in nz], dtype=F)
        _, cnt = np.unique(vals, return_counts=True)
        c["ties"] += int((cnt * (cnt - 1) // 2).sum())
        order = np.array(order_of(s, part), dtype=np.int64)
        sorted_boxes = boxes[order]
        before = s[order].copy()
        overlapped_by_zeroed = np.zeros(order.size, dtype=bool)
        for i in range(order.size):
            if s[order[i]] == 0:                  # `if prob[k] = 0 then continue`
                if chains and before[i] != 0:
                    iou = iou_many(sorted_boxes[i], sorted_boxes[i + 1:])
                    overlapped_by_zeroed[i + 1:] |= iou > thresh
                continue
            iou = iou_many(sorted_boxes[i], sorted_boxes[i + 1:])
            c["near_thresh"] += int((np.abs(iou.astype(D) - D(thresh)) < 1e-5).sum())
            hit = order[i + 1:][iou > thresh]
            c["suppressed"] += int((s[hit] != 0).sum())
            s[hit] = F(0)
        c["chain"] += int((overlapped_by_zeroed & (s[order] != 0)).sum())
    return probs
