"""The detection oracle and cases on the CPU: every case of
tests/_detections_cases.py reaches what it names (from the oracle's counters;
a case that misses fails, it is never skipped), none has a non-zero score tie
or an IoU within 1e-5 of the NMS threshold, the oracle's array arithmetic
agrees with the scalar box_iou the yolo-loss oracle states, values worked by
hand, and the oracle's NMS walk against a second formulation written
independently: per class, sort once, then mark."""
import numpy as np
import pytest

import _detections_cases as cases
import _detections_oracle as oracle
from _yolo_loss_oracle import box_iou

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_case_reaches_what_it_names(name):
    spec, want = cases.build(name), cases.expected(name)
    c = want["counters"]
    for need in spec["needs"]:
        assert c[need] > 0, (name, need, c)
    assert c["ties"] == 0, (name, c)
    assert c["near_thresh"] == 0, (name, c)
    if spec["nms"] is not None:                   # survivors
        assert any((img["probs_nms"] != 0).any() for img in want["images"])


def test_counts_the_cases_are_built_for():
    imgs = cases.expected("3x5_b3")["images"]
    assert imgs[1]["count"] == 0 and imgs[2]["count"] == 3 * 5 * 3 and 0 < imgs[0]["count"] < 45
    assert cases.expected("17x17")["images"][0]["count"] > 512    # rows from >= 3 chunks
    two = cases.expected("two_layers")["images"]
    assert two[0]["layer_counts"][0] != two[1]["layer_counts"][0]
    assert all(min(i["layer_counts"]) > 0 for i in two)
    over = cases.expected("overflow")
    assert all(i["count"] > over["capacity"] for i in over["images"])
    big = cases.expected("nms_52x52")["images"][0]
    assert big["count"] == 52 * 52 * 3
    nonzero = (big["probs"] != 0).sum(axis=0)     # class 0 past the on-chip form, class 1 within
    assert nonzero[0] > cases.NMS_ON_CHIP > nonzero[1] > 0


def test_special_objectness_values():
    img = cases.expected("special")["images"][0]
    c = cases.expected("special")["counters"]
    assert c["nan"] == 2
    inf = np.flatnonzero(np.isinf(img["obj"]))
    assert inf.size == 2
    assert not np.isnan(img["probs"]).any()
    p = img["probs"][inf]
    assert ((p == 0) | np.isinf(p)).all() and (p == 0).any() and np.isinf(p).any()
    assert (img["obj"] > F(cases.THRESH)).all()
    assert (img["obj"] == np.nextafter(F(cases.THRESH), F(1))).sum() == 1
    geo, out = cases.build("special")["layers"][0]
    assert (out[0, :, 4] == F(cases.THRESH)).sum() == 2           # present, and not taken


def test_letterbox_aspects_take_both_branches():
    for name, (im_w, im_h) in cases._ASPECTS.items():
        narrow = (160 / im_w) < (96 / im_h)
        assert narrow == (name == "wide")
        scaled = im_h * 160 / im_w if narrow else im_w * 96 / im_h
        assert scaled != int(scaled)              # the div truncates
    a = cases.expected("boxes_wide_rel0_let0")["images"][0]["boxes"]
    for rel, let in ((0, 1), (1, 0), (1, 1)):
        b = cases.expected(f"boxes_wide_rel{rel}_let{let}")["images"][0]["boxes"]
        assert a.shape == b.shape and not np.array_equal(a, b)


def test_correct_boxes_by_hand():
    # 416 x 416 network, 640 x 480 image, letterbox: 416/640 < 416/480, so
    # new_w = 416, new_h = 480*416 div 640 = 312; deltah = 104, ratioh = 0.75
    b = np.array([[0.5, 0.5, 0.25, 0.375]], dtype=F)
    r = oracle.correct_boxes(b, 640, 480, 416, 416, relative=True, letter=True)
    assert r[0, 0] == F(0.5) and r[0, 2] == F(0.25)
    assert r[0, 1] == F(F(0.5) - F(0.125)) / F(0.75)
    assert r[0, 3] == F(0.375) * F(F(1) / F(0.75))
    r = oracle.correct_boxes(b, 640, 480, 416, 416, relative=False, letter=False)
    assert r.tolist() == [[320.0, 240.0, 160.0, 180.0]]


def test_get_detections_by_hand():
    # one cell, one anchor, two classes
    out = np.array([0.5, 0.25, 0.0, 0.0, 0.5, 0.75, 0.25], dtype=F)
    kw = dict(n=1, classes=2, h=1, w=1, mask=(1,), biases=(1, 1, 16, 8), net_w=32, net_h=32,
              im_w=10, im_h=10, relative=True, letter=False)
    c = oracle.new_counters()
    boxes, obj, probs = oracle.get_detections(out, 0, thresh=0.25, counters=c, **kw)
    assert boxes.tolist() == [[0.5, 0.25, 0.5, 0.25]] and obj.tolist() == [0.5]
    assert probs.tolist() == [[0.375, 0.0]] and c["taken"] == 1 and c["zeroed_prob"] == 1
    boxes, obj, probs = oracle.get_detections(out, 0, thresh=0.5, **kw)       # strict
    assert obj.size == 0 and boxes.shape == (0, 4) and probs.shape == (0, 2)


def test_iou_many_is_the_scalar_box_iou():
    img = cases.expected("nms_5x7")["images"][0]
    boxes = img["boxes"]
    for i in range(0, boxes.shape[0], 7):
        many = oracle.iou_many(boxes[i], boxes)
        one = np.array([box_iou(tuple(boxes[i]), tuple(b)) for b in boxes], dtype=F)
        assert np.array_equal(_bits(many), _bits(one))
    assert (oracle.iou_many(boxes[0], boxes) > 0).sum() > 1


def _nms_second_formulation(boxes, obj, probs, thresh):
    """Per class: sort once by (score descending, row ascending), then mark:
    a row is kept when it is non-zero and no kept row before it overlaps it
    above thresh; every other row is 0.  Scalar IoUs."""
    res = np.array(probs, dtype=F)
    rows = [r for r in range(len(obj)) if obj[r] != 0]
    for k in range(res.shape[1]):
        col = res[:, k].copy()
        order = sorted(rows, key=lambda r: (-float(col[r]), r))
        kept = []
        for r in order:
            if col[r] == 0:
                continue
            if any(box_iou(tuple(boxes[q]), tuple(boxes[r])) > F(thresh) for q in kept):
                res[r, k] = 0
            else:
                kept.append(r)
    return res


@pytest.mark.parametrize("name", ["nms_5x7", "nms_13x13", "nms_3x5_80cls", "overflow"])
def test_nms_against_second_formulation(name):
    want = cases.expected(name)
    for img in want["images"]:
        m = min(img["count"], want["capacity"])
        other = _nms_second_formulation(img["boxes"][:m], img["obj"][:m], img["probs"][:m],
                                        cases.NMS)
        assert np.array_equal(_bits(other), _bits(img["probs_nms"]))


def test_nms_by_hand():
    # A (0.9) overlaps B (0.8) above 0.45, B overlaps C (0.7), A does not reach
    # C: B is zeroed and suppresses nothing, so C survives (a chain)
    boxes = np.array([[0.0, 0, 2, 2], [0.5, 0, 2, 2], [1.0, 0, 2, 2], [9, 9, 1, 1]], dtype=F)
    probs = np.array([[0.9], [0.8], [0.7], [0.6]], dtype=F)
    c = oracle.new_counters()
    r = oracle.nms_sort(boxes, np.ones(4, dtype=F), probs, 0.45, counters=c)
    assert r[:, 0].tolist() == [F(0.9), 0.0, F(0.7), F(0.6)]
    assert c["suppressed"] == 1 and c["chain"] == 1 and c["ties"] == 0
    # the tie rule: equal scores, the lower row first
    r = oracle.nms_sort(boxes[[1, 0]], np.ones(2, dtype=F), np.array([[0.5], [0.5]], dtype=F),
                        0.45, counters=c)
    assert r[:, 0].tolist() == [0.5, 0.0] and c["ties"] == 1


def test_zero_objectness_rows_stay_out():
    boxes, obj, probs, after, c = cases.zero_objectness_rows()
    zero = obj == 0
    assert c["zero_obj"] == zero.sum() > 3 and c["suppressed"] > 0 and c["ties"] == 0
    assert np.signbit(obj[zero]).any() and not np.signbit(obj[zero]).all()
    assert np.array_equal(_bits(after[zero]), _bits(probs[zero]))      # not suppressed
    alone = oracle.nms_sort(boxes[~zero], obj[~zero], probs[~zero], cases.NMS)
    assert np.array_equal(_bits(after[~zero]), _bits(alone))           # and suppress nothing
    # they would, had they taken part: their scores are the largest
    every = oracle.nms_sort(boxes, np.ones_like(obj), probs, cases.NMS)
    assert not np.array_equal(_bits(every[~zero]), _bits(alone))
