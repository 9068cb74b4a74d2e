"""The device yolo loss off the GPU: the plan fields it reads, the refusals
of HipDarknetTrain(yolo_loss=True), the NumPy oracle on cases worked by hand,
and the GPU test's inputs held against their coverage conditions by the
oracle's counters alone."""
import math

import numpy as np
import pytest

from tensorium_amd import darknet as dn

import _yolo_loss_cases as cases
from _yolo_loss_oracle import COUNTERS, sum_sqr, yolo_loss

F = np.float32
V3 = (10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326)
TINY = (10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319)


def _yolos(cfg, **kw):
    net = dn.Network(dn.parse_cfg(cfg), **kw)
    return net, [l for l in net.layers if l.kind == "yolo"]


@pytest.mark.parametrize("cfg,anchors,masks", [
    (dn.yolov3_cfg(64, batch=2, classes=3), V3, [(6, 7, 8), (3, 4, 5), (0, 1, 2)]),
    (dn.yolov3_tiny_cfg(64, batch=2, classes=3), TINY, [(3, 4, 5), (0, 1, 2)])])
def test_plan_fields_of_the_sample_networks(cfg, anchors, masks):
    net, ys = _yolos(cfg)
    assert [l.mask for l in ys] == masks
    assert net.yolo_unbuilt == ()
    for l in ys:
        assert l.anchors == 3 and l.total == len(anchors) // 2   # anchors stays the count
        assert l.biases == tuple(float(a) for a in anchors)
        assert l.max_boxes == 200
        assert l.ignore_thresh == float(F(0.7)) and l.truth_thresh == 1.0
        assert l.iou_thresh == 1.0 and l.iou_normalizer == 0.75
        assert l.obj_normalizer == 1.0 and l.delta_normalizer == 1.0
        assert l.unbuilt == ()


HEAD = "[net]\nbatch=1\nwidth=32\nheight=32\nchannels=3\n"
CONV = "[convolutional]\nfilters=16\nsize=1\nstride=1\nactivation=linear\n"  # 2 * (3 + 5)


def test_plan_fields_every_key_set_and_defaults():
    cfg = (HEAD + CONV + "[yolo]\nmask=1,3\nnum=4\nclasses=3\nanchors=1.5,2, 3,4.25, 5\nmax=7\n"
           "ignore_thresh=.3\ntruth_thresh=.9\niou_thresh=.213\niou_normalizer=.07\n"
           "obj_normalizer=.4\ndelta_normalizer=2.5\n")
    _, (l,) = _yolos(cfg)
    assert l.mask == (1, 3) and l.anchors == 2 and l.total == 4 and l.max_boxes == 7
    # absent anchors keep the constructor's fill of 0.5
    assert l.biases == (1.5, 2.0, 3.0, 4.25, 5.0, 0.5, 0.5, 0.5)
    got = (l.ignore_thresh, l.truth_thresh, l.iou_thresh, l.iou_normalizer, l.obj_normalizer,
           l.delta_normalizer)
    assert got == tuple(float(F(v)) for v in (.3, .9, .213, .07, .4, 2.5))
    # the parser's defaults (nparser.pas:516-643)
    _, (l,) = _yolos(HEAD + CONV.replace("16", "8") + "[yolo]\nmask=0\nclasses=3\n")
    assert (l.total, l.biases, l.max_boxes) == (1, (0.5, 0.5), 200)
    assert (l.ignore_thresh, l.truth_thresh, l.iou_thresh) == (0.5, 1.0, 1.0)
    assert (l.iou_normalizer, l.obj_normalizer, l.delta_normalizer) == (0.75, 1.0, 1.0)


class _NoDevice:
    """Stands where torch would: a refusal comes before any allocation."""

    def __getattr__(self, name):
        raise AssertionError(f"torch.{name} reached before the refusal")


def _train(cfg, **kw):
    net = dn.Network(dn.parse_cfg(cfg))
    return dn.HipDarknetTrain(None, net, dn.random_params(net, seed=1), _NoDevice(), **kw)


YOLO = "[yolo]\nmask=0,1\nnum=2\nclasses=3\nanchors=4,4,8,8\n"


@pytest.mark.parametrize("where,line,key", [
    ("yolo", "iou_loss=giou", "iou_loss"), ("yolo", "iou_thresh_kind=giou", "iou_thresh_kind"),
    ("yolo", "focal_loss=1", "focal_loss"), ("yolo", "objectness_smooth=1", "objectness_smooth"),
    ("yolo", "label_smooth_eps=0.1", "label_smooth_eps"), ("yolo", "new_coords=1", "new_coords"),
    ("yolo", "counters_per_class=5,6,7", "counters_per_class"), ("yolo", "map=coco9k.map", "map"),
    ("yolo", "embedding_layer=-2", "embedding_layer"), ("yolo", "scale_x_y=1.05", "scale_x_y"),
    ("net", "adversarial_lr=0.05", "adversarial_lr"), ("net", "adversarial=1", "adversarial"),
    ("net", "equidistant_point=100", "equidistant_point"),
    ("net", "badlabels_rejection_percentage=0.2", "badlabels_rejection_percentage"),
    ("net", "num_sigmas_reject_badlabels=3", "num_sigmas_reject_badlabels")])
def test_yolo_loss_refuses_what_is_not_built(where, line, key):
    head = HEAD + (line + "\n" if where == "net" else "")
    cfg = head + CONV + YOLO + (line + "\n" if where == "yolo" else "")
    with pytest.raises(ValueError, match=rf"\b{key}\b"):
        _train(cfg, yolo_loss=True)
    # refused only there: the plan, and the existing training path, take it
    with pytest.raises(AssertionError, match="reached before the refusal"):
        _train(cfg)


def test_yolo_loss_refuses_unequal_max():
    cfg = HEAD + CONV + YOLO + "max=30\n" + "[route]\nlayers=-2\n" + CONV + YOLO + "max=40\n"
    with pytest.raises(ValueError, match=r"\bmax\b"):
        _train(cfg, yolo_loss=True)


def _kw(**over):
    kw = dict(batch=1, n=1, classes=2, h=2, w=2, total=1, mask=(0,), biases=(32.0, 32.0),
              max_boxes=3, net_w=64, net_h=64, ignore_thresh=0.5, truth_thresh=1.0,
              iou_thresh=1.0, iou_normalizer=0.75, obj_normalizer=1.0)
    kw.update(over)
    return kw


def test_oracle_no_truths():
    rng = np.random.default_rng(5)
    out = rng.uniform(0.05, 0.95, (2, 2, 7, 6)).astype(F)    # batch 2, 2 anchors, 2 classes, 2x3
    kw = _kw(batch=2, n=2, total=2, mask=(0, 1), biases=(8., 8., 16., 16.), h=2, w=3)
    r = yolo_loss(out, np.zeros((2, 18), dtype=F), **kw)
    want = np.zeros_like(out)
    want[:, :, 4] = -out[:, :, 4]
    assert np.array_equal(r["delta"].reshape(out.shape), want)
    s = F(0)
    for v in out[:, :, 4].reshape(-1):    # the objectness planes in index order
        s = F(s + F(v * v))
    assert r["cost"] == s == sum_sqr(want)
    assert r["total_bbox"] == 0 and not r["stats"].any() and not any(r["counters"].values())
    assert np.array_equal(r["output"], out.reshape(-1))


def test_oracle_one_centred_truth_by_hand():
    # 2x2 grid of a 64x64 network, one anchor of 32x32 (0.5 of the image).
    # The truth sits in the middle of cell (col 1, row 0) with the anchor's
    # shape; every cell predicts its own centre with the anchor's shape, so
    # that cell's box is the truth's (IoU 1), objectness 0.5, classes 0.125.
    out = np.zeros((1, 1, 7, 4), dtype=F)
    out[0, 0, 0:2] = 0.5
    out[0, 0, 4] = 0.5
    out[0, 0, 5:] = 0.125
    truth = np.zeros((1, 3, 6), dtype=F)
    truth[0, 0] = (0.75, 0.25, 0.5, 0.5, 1, 9)
    r = yolo_loss(out, truth, **_kw())
    d = r["delta"].reshape(7, 4)
    cell = 1                                    # row 0, col 1
    # scale = 2 - 0.5*0.5; tx - out = 0.75*2 - 1 - 0.5 = 0; tw = ln(0.5*2/32)
    assert d[0, cell] == 0 and d[1, cell] == 0
    dw = 1.75 * math.log(1 / 32) * 0.75
    assert d[2, cell] == pytest.approx(dw, rel=1e-6) and d[3, cell] == d[2, cell]
    assert d[4, cell] == 0.5                    # obj_normalizer * (1 - 0.5)
    assert d[5, cell] == -0.125 and d[6, cell] == 0.875
    others = [c for c in range(4) if c != cell]
    assert (d[4, others] == -0.5).all()         # below ignore_thresh, or no class above 0.25
    assert not d[[0, 1, 2, 3, 5, 6]][:, others].any()
    assert r["stats"].tolist() == [[1.0, 1.0]]  # count, tot_iou
    assert (r["total_bbox"], r["rewritten_bbox"]) == (1, 0)
    assert r["counters"]["truth_writes"] == 1 and r["counters"]["unmatched"] == 1
    assert r["cost"] == sum_sqr(d)
    # class scores above 0.25: the matched cell is zeroed by ignore_thresh
    # first; truth_thresh below the IoU takes the cell in the cell pass too
    out[0, 0, 5:] = 0.5
    r2 = yolo_loss(out, truth, **_kw(truth_thresh=0.9))
    assert r2["counters"]["ignored"] == 1 and r2["counters"]["truth_thresh"] == 1
    assert r2["rewritten_bbox"] == 1 and r2["total_bbox"] == 2
    d2 = r2["delta"].reshape(7, 4)
    # the box deltas accumulate over the two passes; the class delta of the
    # truth's class, already non-zero, is the only one rewritten
    assert d2[2, cell] == F(d[2, cell] + d[2, cell])
    assert d2[5, cell] == -0.5 and d2[6, cell] == 0.5


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_case_reaches_its_branches(name):
    counters = cases.expected(name)["counters"]
    assert counters["out_of_grid"] == 0          # that guard is read, not exercised
    for need in cases.CASES[name]["needs"]:
        assert counters[need] > 0, (name, need, counters)


def test_cases_cover_every_counter_and_shape():
    total = {k: sum(cases.expected(n)["counters"][k] for n in cases.CASES)
             for k in COUNTERS + ("unmatched",)}
    assert all(v > 0 for v in total.values()), total
    kws = [cases.kwargs_of(n) for n in cases.CASES]
    assert {(k["h"], k["w"]) for k in kws} >= {(3, 5), (13, 13), (2, 3)}
    assert any(k["h"] * k["w"] > 256 for k in kws)     # more than one block of cells
    assert {(k["mask"], k["total"]) for k in kws} == {((0, 1, 2), 6), ((3, 4, 5), 6),
                                                       ((6, 7, 8), 9)}
    assert {k["batch"] for k in kws} == {1, 3} and {k["max_boxes"] for k in kws} == {4, 200}
    assert {k["classes"] for k in kws} == {3, 80}
    assert {k["truth_thresh"] for k in kws} == {1.0, float(F(0.7))}
    assert {k["iou_thresh"] for k in kws} == {1.0, float(F(0.2))}
