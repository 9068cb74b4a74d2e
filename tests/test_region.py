"""[region] in the layer plan (parseRegion, nparser.pas:646-712) and the
region oracle on a loss small enough to work out by hand.  No GPU."""
import numpy as np
import pytest

from tensorium_amd import darknet as dn

import _region_oracle as ro

F = np.float32


def _plan(region, filters=125):
    cfg = ("[net]\nheight=8\nwidth=8\nchannels=3\n[convolutional]\n"
           f"filters={filters}\nsize=1\nactivation=linear\n[region]\n" + region)
    return dn.Network(dn.parse_cfg(cfg)).layers[-1]


def _keys(l):
    return (l.max_boxes, l.softmax, l.rescore, l.bias_match, l.classfix, l.thresh, l.coord_scale,
            l.object_scale, l.noobject_scale, l.class_scale)


def test_region_plans_with_defaults_and_every_key():
    l = _plan("num=5\n")
    assert (l.kind, l.c, l.h, l.w, l.out_size, l.anchors, l.classes) == \
        ("region", 125, 8, 8, 125 * 64, 5, 20)
    assert _keys(l) == (200, 0, 0, 0, 0, 0.5, 1, 1, 1, 1)
    assert l.biases == (0.5,) * 10
    l = dn.Network(dn.parse_cfg(dn.tiny_yolo_voc_cfg(416) + "max=30\nclassfix=2\n")).layers[-1]
    assert (l.kind, l.c, l.h, l.w) == ("region", 125, 13, 13)
    assert _keys(l) == (30, 1, 1, 1, 2, float(F(0.6)), 1, 5, 1, 1)
    assert l.biases == tuple(float(F(v)) for v in (1.08, 1.19, 3.42, 4.41, 6.63, 11.38, 9.42,
                                                   5.11, 16.62, 10.52))
    assert _plan("num=5\nanchors=1.5,2\n").biases == (1.5, 2.0) + (0.5,) * 8


@pytest.mark.parametrize("region, filters, match", [
    ("num=5\ntree=data/9k.tree\n", 125, "tree="), ("num=5\nmap=data/coco9k.map\n", 125, "map="),
    ("num=5\nfocal_loss=1\n", 125, "focal_loss"), ("num=5\nclasses=19\ncoords=5\n", 125, "coords="),
    ("num=5\n", 120, "doesn't correspond to classes= or num=")])
def test_region_refusals(region, filters, match):
    with pytest.raises(ValueError, match=match):
        _plan(region, filters)


def test_one_cell_loss_by_hand():
    """1x1 grid, one anchor (bias 1, 1), seen past the prior stage.  Raw box
    entries 0 predict (0.5, 0.5, 1, 1), the truth is that box with class 1: box
    deltas 0, objectness (1 - 0.5) * 0.25, classes -0.25 and 0.25."""
    delta, cost = ro.loss(np.array([0, 0, 0, 0, 0.5, 0.25, 0.75], F),
                          np.array([[0.5, 0.5, 1, 1, 1, 0], [0] * 6], F), batch=1, num=1,
                          classes=2, h=1, w=1, biases=(1, 1), max_boxes=2, seen=12800)
    assert delta.tolist() == [0, 0, 0, 0, 0.125, -0.25, 0.25]
    assert cost == F(0.140625) * F(0.140625)
