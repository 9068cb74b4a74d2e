"""TRegionLayer (nregionlayer.pas) restated with NumPy scalars in FPC's typing
(exp / ln return a real, rounded where Pascal assigns a single): forward, loss
and getDetections, the built branches only, with the departures DESIGN.md states."""
import numpy as np

from _detections_oracle import correct_boxes
from _yolo_loss_oracle import D, F, _trunc, box_iou, sum_sqr


def same_bits(got, want, what):
    got, want = (np.asarray(v.cpu() if hasattr(v, "cpu") else v, F).reshape(-1)
                 for v in (got, want))
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def logistic(x):
    return F(D(1) / (D(1) + np.exp(D(F(-F(x))))))


def gradient(x):
    return F(F(F(1) - x) * x)


def forward(inp, batch, num, classes, hw, softmax):
    """[batch][num*size][hw] -> [batch][hw][num][size], activated."""
    size = classes + 5
    out = np.ascontiguousarray(
        np.array(inp, F).reshape(batch, num * size, hw).transpose(0, 2, 1)).reshape(-1, size)
    for cell in out:
        cell[4] = logistic(cell[4])
        if softmax and classes:
            x = cell[5:]
            largest = x[0]
            for v in x[1:]:
                if v > largest:
                    largest = v
            s = F(0)
            for i in range(classes):
                e = F(np.exp(D(F(F(x[i] - largest) / F(1)))))
                s = F(s + e)
                x[i] = e
            for i in range(classes):
                x[i] = F(x[i] / s)
    return out.reshape(-1)


def get_box(o, bias, n, col, row, w, h):
    return (F(F(F(col) + logistic(o[0])) / F(w)), F(F(F(row) + logistic(o[1])) / F(h)),
            F(np.exp(D(o[2])) * D(bias[2 * n]) / D(w)),
            F(np.exp(D(o[3])) * D(bias[2 * n + 1]) / D(h)))


def delta_box(truth, o, d, bias, n, col, row, w, h, scale):
    iou = box_iou(get_box(o, bias, n, col, row, w, h), truth)
    tx, ty = F(F(truth[0] * F(w)) - F(col)), F(F(truth[1] * F(h)) - F(row))
    tw = F(np.log(D(F(F(truth[2] * F(w)) / bias[2 * n]))))
    th = F(np.log(D(F(F(truth[3] * F(h)) / bias[2 * n + 1]))))
    lx, ly = logistic(o[0]), logistic(o[1])
    d[0] = F(F(scale * F(tx - lx)) * gradient(lx))
    d[1] = F(F(scale * F(ty - ly)) * gradient(ly))
    d[2], d[3] = F(scale * F(tw - o[2])), F(scale * F(th - o[3]))
    return iou


def _rows(truth_b, classes):
    for r in truth_b:  # class >= classes is skipped before the x = 0 break
        if not r[4] < classes:
            continue
        if r[0] == 0:
            break
        yield r, -1 if r[4] <= -1 else _trunc(r[4])


def loss(out, truth, *, batch, num, classes, h, w, biases, max_boxes, seen, rescore=False,
         bias_match=False, classfix=0, thresh=0.5, coord_scale=1, object_scale=1,
         noobject_scale=1, class_scale=1):
    """Returns delta [batch][num*size][h*w] (un-flattened) and cost."""
    size, bias = classes + 5, np.asarray(biases, F)
    sc = dict(thresh=F(thresh), coord=F(coord_scale), obj=F(object_scale),
              noobj=F(noobject_scale), cls=F(class_scale))
    out = np.asarray(out, F).reshape(batch, h * w * num, size)
    truth = np.asarray(truth, F).reshape(batch, max_boxes, 6)
    delta = np.zeros_like(out)
    for b in range(batch):
        for j in range(h):
            for i in range(w):
                for n in range(num):
                    o, d = out[b, (j * w + i) * num + n], delta[b, (j * w + i) * num + n]
                    pred = get_box(o, bias, n, i, j, w, h)
                    best_iou, best_cls = F(0), -1
                    for r, cls in _rows(truth[b], classes):
                        iou = box_iou(pred, r[:4])
                        if iou > best_iou:
                            best_cls, best_iou = cls, iou
                    d[4] = F(sc["noobj"] * F(F(-o[4]) * gradient(o[4])))
                    if classfix == -1:
                        d[4] = F(sc["noobj"] * F(F(best_iou - o[4]) * gradient(o[4])))
                    elif best_iou > sc["thresh"]:
                        d[4] = 0
                        if classfix > 0:
                            cs = F(sc["cls"] * (o[4] if classfix == 2 else F(1)))
                            for c in range(classes):
                                d[5 + c] = F(cs * F(F(1 if c == best_cls else 0) - o[5 + c]))
                    if seen < 12800:
                        prior = (F(F(F(i) + F(0.5)) / F(w)), F(F(F(j) + F(0.5)) / F(h)),
                                 F(bias[2 * n] / F(w)), F(bias[2 * n + 1] / F(h)))
                        delta_box(prior, o, d, bias, n, i, j, w, h, F(0.01))
        for r, cls in _rows(truth[b], classes):
            fi, fj = F(r[0] * F(w)), F(r[1] * F(h))
            if not (-1 < fi < w and -1 < fj < h):
                continue                                   # departure: outside the grid
            i, j = _trunc(fi), _trunc(fj)
            best_iou, best_n = F(0), 0
            for n in range(num):
                pred = get_box(out[b, (j * w + i) * num + n], bias, n, i, j, w, h)
                if bias_match:
                    pred = (0, 0, F(bias[2 * n] / F(w)), F(bias[2 * n + 1] / F(h)))
                iou = box_iou((F(0), F(0), pred[2], pred[3]), (F(0), F(0), r[2], r[3]))
                if iou > best_iou:
                    best_iou, best_n = iou, n
            o, d = out[b, (j * w + i) * num + best_n], delta[b, (j * w + i) * num + best_n]
            iou = delta_box(r[:4], o, d, bias, best_n, i, j, w, h, sc["coord"])
            d[4] = F(F(sc["obj"] * F(F(1) - o[4])) * gradient(o[4]))
            if rescore:
                d[4] = F(F(sc["obj"] * F(iou - o[4])) * gradient(o[4]))
            for c in range(classes):
                d[5 + c] = F(sc["cls"] * F(F(1 if c == cls else 0) - o[5 + c]))
    delta = np.ascontiguousarray(delta.reshape(batch, h * w, num * size).transpose(0, 2, 1))
    s = sum_sqr(delta)
    return delta.reshape(-1), F(s * s)


def detections(out, b, *, num, classes, h, w, biases, classfix, net_w, net_h, im_w, im_h, thresh,
               relative, letter):
    """Image b's rows: (boxes [m, 4], objectness [m], probs [m, classes])."""
    size, bias = classes + 5, np.asarray(biases, F)
    out = np.asarray(out, F).reshape(-1, h * w * num, size)[b]
    boxes, probs = [], []
    for u, o in enumerate(out):
        scale = F(0) if classfix == -1 and o[4] < 0.5 else o[4]
        p = np.zeros(classes, F)
        for j in range(classes):
            v = F(scale * o[5 + j])
            p[j] = v if v > F(thresh) else 0
        if p.any():                                        # departure: empty rows dropped
            cell = u // num
            boxes.append(get_box(o, bias, u % num, cell % w, cell // w, w, h))
            probs.append(p)
    m = len(boxes)
    return (correct_boxes(np.array(boxes, F).reshape(m, 4), im_w, im_h, net_w, net_h, relative,
                          letter), np.ones(m, F), np.array(probs, F).reshape(m, classes))
