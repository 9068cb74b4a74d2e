"""The inputs of tests/test_gpu_detections.py: [yolo] layers' activated
outputs, built so that every behaviour of tns_hip_yolo_detections /
tns_hip_nms_sort named in CASES is reached.  tests/test_detections.py proves
on the CPU, from the oracle's counters (``needs``), that each case reaches
what it names, and that none has a non-zero score tie or an IoU within 1e-5
of the NMS threshold: in both the reference's answer is unspecified or one
rounding from flipping.  Expected results come from tests/_detections_oracle.py,
computed once per case.

The construction: x, y ~ U(0.1, 0.9); w, h ~ N(0, 0.3); objectness and class
scores ~ U(0, 1); the yolov3-tiny anchors with mask 3,4,5; a 32*w x 32*h
network; thresh 0.25, NMS 0.45.
"""
import functools

import numpy as np

import _detections_oracle as oracle

F = np.float32
ANCHORS = (10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319)
THRESH, NMS = 0.25, 0.45
NMS_ON_CHIP = 2048      # kNmsLds, csrc/detections.hip: sorted in LDS up to here


def layer(seed, batch, h, w, classes, n=3, obj=None, mask=(3, 4, 5)):
    """One layer: its geometry keywords and its output [batch][n][classes+5][h*w].
    obj: per image, None (uniform), "none" (all below THRESH) or "all" (all above)."""
    rng = np.random.default_rng(seed)
    out = np.empty((batch, n, classes + 5, h * w), dtype=F)
    out[:, :, 0:2] = rng.uniform(0.1, 0.9, (batch, n, 2, h * w))
    out[:, :, 2:4] = rng.normal(0.0, 0.3, (batch, n, 2, h * w))
    out[:, :, 4:] = rng.uniform(0.0, 1.0, (batch, n, classes + 1, h * w))
    for b, kind in enumerate(obj or ()):
        if kind == "none":
            out[b, :, 4] *= F(0.2)
        elif kind == "all":
            out[b, :, 4] = F(0.3) + F(0.7) * out[b, :, 4]
    geo = dict(n=n, classes=classes, h=h, w=w, total=6, mask=mask, biases=ANCHORS)
    return geo, out


def _big():
    """52 x 52, the small anchors, every objectness above thresh: 8112 rows.
    Class 0 has more non-zero scores than the on-chip NMS form holds, class 1
    (scores scaled by 0.4) fewer, so one launch takes both forms."""
    geo, out = layer(202, 1, 52, 52, 2, obj=("all",), mask=(0, 1, 2))
    out[0, :, 6] *= F(0.4)
    return geo, out


def _special():
    geo, out = layer(41, 1, 3, 5, 3)
    o = out[0]
    o[0, 4, 2] = np.nan                 # not taken
    o[1, 4, 7] = np.nan
    o[2, 4, 4] = np.inf                 # taken: Inf * score = Inf, Inf * 0 = NaN -> 0
    o[2, 5, 4] = 0.0
    o[0, 4, 9] = np.inf
    o[1, 4, 11] = F(THRESH)             # exactly thresh: not taken
    o[2, 4, 0] = F(THRESH)
    o[0, 4, 13] = np.nextafter(F(THRESH), F(1))   # the next single above: taken
    return geo, out


def _spec(layers, batch, net=None, im=(517, 389), relative=False, letter=False, capacity=None,
          nms=None, needs=("taken",), chains=True):
    g = layers[0][0]
    return dict(layers=layers, batch=batch, net=net or (32 * g["w"], 32 * g["h"]), im=im,
                relative=relative, letter=letter, capacity=capacity, nms=nms, needs=needs,
                chains=chains, thresh=THRESH)


# two image aspects, one on each side of netw/w < neth/h for the 160 x 96
# network, neither a multiple of it: (901, 333) scales by width, new_h =
# 333*160 div 901 = 59 (59.13..); (517, 389) by height, new_w = 517*96 div 389
# = 127 (127.58..)
_ASPECTS = {"wide": (901, 333), "tall": (517, 389)}

CASES = {
    # h != w; image 1 has nothing above thresh, image 2 every candidate
    "3x5_b3": lambda: _spec([layer(11, 3, 3, 5, 4, obj=(None, "none", "all"))], 3,
                            needs=("taken", "zeroed_prob")),
    # 867 candidates: four chunks of 256, so the compaction spans waves and workgroups
    "17x17": lambda: _spec([layer(12, 1, 17, 17, 3)], 1),
    "2x3_80cls": lambda: _spec([layer(13, 2, 2, 3, 80)], 2, needs=("taken", "zeroed_prob")),
    "2x3_1cls": lambda: _spec([layer(14, 2, 2, 3, 1)], 2),
    # 3x5 then 6x10 through counts; the images' counts differ
    "two_layers": lambda: _spec([layer(15, 2, 3, 5, 4), layer(16, 2, 6, 10, 4)], 2,
                                net=(160, 96)),
    # capacity below the count, then NMS over the rows that fitted
    "overflow": lambda: _spec([layer(17, 2, 5, 7, 4)], 2, capacity=20, nms=NMS,
                              needs=("taken", "suppressed")),
    "special": lambda: _spec([_special()], 1, needs=("taken", "nan")),
    # the dense layer: suppressions, chains (a zeroed row suppresses nothing)
    "nms_5x7": lambda: _spec([layer(18, 1, 5, 7, 4)], 1, nms=NMS,
                             needs=("taken", "suppressed", "chain")),
    "nms_13x13": lambda: _spec([layer(100, 1, 13, 13, 3)], 1, nms=NMS,
                               needs=("taken", "suppressed", "chain")),
    "nms_3x5_80cls": lambda: _spec([layer(20, 2, 3, 5, 80)], 2, nms=NMS,
                                   needs=("taken", "suppressed", "chain")),
    # 8112 rows, all taken: more non-zero scores in class 0 than the on-chip form holds
    "nms_52x52": lambda: _spec([_big()], 1, nms=NMS,
                               needs=("taken", "suppressed"), chains=False),
}
for _a, _im in _ASPECTS.items():
    for _rel in (False, True):
        for _let in (False, True):
            CASES[f"boxes_{_a}_rel{int(_rel)}_let{int(_let)}"] = (
                lambda im=_im, rel=_rel, let=_let: _spec([layer(22, 2, 3, 5, 4)], 2, im=im,
                                                         relative=rel, letter=let))


@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name]()


def default_capacity(spec):
    return sum(g["n"] * g["h"] * g["w"] for g, _ in spec["layers"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """Per image: the full count, the rows in order (all of them, fitting or
    not), and with ``nms`` the probs after NMS over the rows that fitted."""
    spec = build(name)
    cap = spec["capacity"] or default_capacity(spec)
    c = oracle.new_counters()
    images = []
    for b in range(spec["batch"]):
        parts = [oracle.get_detections(out, b, net_w=spec["net"][0], net_h=spec["net"][1],
                                       im_w=spec["im"][0], im_h=spec["im"][1],
                                       thresh=spec["thresh"], relative=spec["relative"],
                                       letter=spec["letter"], counters=c, **geo)
                 for geo, out in spec["layers"]]
        boxes, obj, probs = (np.concatenate([p[k] for p in parts]) for k in range(3))
        img = dict(count=obj.size, layer_counts=[p[1].size for p in parts], boxes=boxes, obj=obj,
                   probs=probs)
        if spec["nms"] is not None:
            m = min(obj.size, cap)
            img["probs_nms"] = oracle.nms_sort(boxes[:m], obj[:m], probs[:m], spec["nms"],
                                               counters=c, chains=spec["chains"])
        images.append(img)
    return dict(images=images, counters=c, capacity=cap)


@functools.lru_cache(maxsize=None)
def zero_objectness_rows():
    """Rows for tns_hip_nms_sort alone: the dense 5x7 layer's, with every
    third row's objectness set to 0 (+0 and -0 by turns) and its scores to 5,
    above every other score.  Such rows must neither suppress nor be
    suppressed.  Returns (boxes, objectness, probs, probs after NMS, counters)."""
    img = expected("nms_5x7")["images"][0]
    boxes, obj, probs = img["boxes"].copy(), img["obj"].copy(), img["probs"].copy()
    for i, r in enumerate(range(0, obj.size, 3)):
        obj[r] = F(0.0) if i % 2 == 0 else F(-0.0)
        probs[r] = F(5)
    c = oracle.new_counters()
    after = oracle.nms_sort(boxes, obj, probs, NMS, counters=c)
    return boxes, obj, probs, after, c
