"""Decoded images in, detections or the yolo loss out, on yolov3-tiny:
HipDarknet.detect_images and HipDarknetTrain.load_batch against the same
network fed the oracle's preprocessed input (tests/_image_oracle.py).  The
network is deterministic, so equal rows, deltas and costs say that the device
preprocessing left the oracle's bits in the input; the input is compared
directly as well."""
import numpy as np
import pytest

from tensorium_amd import darknet as dn

import _image_oracle as oracle

pytestmark = pytest.mark.gpu
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _net():
    return dn.Network(dn.parse_cfg(dn.yolov3_tiny_cfg(size=64, batch=2, classes=2)))


def _bytes(rng, w, h):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _objectness(ys, outs):
    return np.concatenate([o.reshape(2, l.anchors, l.classes + 5, -1)[:, :, 4].reshape(-1)
                           for l, o in zip(ys, outs)])


def _same_rows(got, want):
    assert len(got) == len(want) == 2
    for b, (g, w) in enumerate(zip(got, want)):
        for u, v, name in zip(g, w, ("boxes", "objectness", "probs")):
            assert u.shape == v.shape, (b, name, u.shape, v.shape)
            assert np.array_equal(_bits(u), _bits(v)), (b, name)


def test_detect_images(hip, torch_cuda):
    torch = torch_cuda
    net = _net()
    ys = [l for l in net.layers if l.kind == "yolo"]
    assert [(l.h, l.w) for l in ys] == [(2, 2), (4, 4)] and (net.w, net.h, net.c) == (64, 64, 3)
    A = dn.HipDarknet(hip, net, dn.random_params(net, seed=91), torch)
    rng = np.random.default_rng(92)

    def fed_the_oracle(X, im, letter, relative, nms):
        """forward + detections on the oracle's input; thresh: a quantile of
        its objectness values, so that rows pass whatever the parameters give"""
        x = torch.from_numpy(np.ascontiguousarray(np.stack(X))).cuda()
        A.forward(x)
        hip.finish()
        outs = [A.out[l.index].cpu().numpy() for l in ys]
        thresh = float(F(np.quantile(_objectness(ys, outs), 0.6)))
        want = A.detections(im[0], im[1], thresh=thresh, relative=relative, letter=letter, nms=nms)
        rows = [w[1].size for w in want]
        print("thresh", thresh, "rows", rows)
        assert min(rows) > 0 and 20 <= sum(rows) <= 60, rows   # 120 candidates, 40 % of them
        return thresh, want

    # the sample's mode: resize, relative boxes; two sizes in one batch
    mixed = [_bytes(rng, 50, 40), _bytes(rng, 33, 71)]
    X = [oracle.resize(oracle.planar_from_bytes(im, 3), 64, 64) for im in mixed]
    for nms in (None, 0.45):
        thresh, want = fed_the_oracle(X, (50, 40), False, True, nms)
        got = A.detect_images(mixed, thresh=thresh, nms=nms)
        _same_rows(got, want)
    x, placed = A.load_images(mixed)
    hip.finish()
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(np.stack(X)))
    assert [(p.new_w, p.new_h, p.dx, p.dy, p.w, p.h, p.ratio) for p in placed] == \
        [(64, 64, 0, 0, 50, 40, None), (64, 64, 0, 0, 33, 71, None)]

    # letterbox: one size, the boxes corrected for it, absolute
    equal = [_bytes(rng, 50, 20), _bytes(rng, 50, 20)]
    X = [oracle.letterbox(oracle.planar_from_bytes(im, 3), 64, 64)[0] for im in equal]
    thresh, want = fed_the_oracle(X, (50, 20), True, False, 0.45)
    got = A.detect_images(equal, thresh=thresh, nms=0.45, letter=True, relative=False)
    _same_rows(got, want)

    # mixed sizes where the boxes depend on the image extent
    for kw in (dict(letter=True), dict(relative=False)):
        with pytest.raises(ValueError, match="differing sizes"):
            A.detect_images(mixed, thresh=thresh, **kw)
    with pytest.raises(ValueError, match="1 images for a batch of 2"):
        A.load_images(mixed[:1])


def test_load_batch_feeds_the_yolo_loss(hip, torch_cuda):
    torch = torch_cuda
    net = _net()
    ys = [l for l in net.layers if l.kind == "yolo"]
    params = dn.random_params(net, seed=93)
    rng = np.random.default_rng(94)
    images = [_bytes(rng, 50, 20), _bytes(rng, 37, 53)]
    boxes = [[(5, 2, 40, 18, 1), (20, 5, 30, 12, 0)], [(3, 10, 30, 50, 1)]]
    X, rows = [], []
    for im, objs in zip(images, boxes):
        x, (_, _, dx, dy, ratio) = oracle.letterbox(oracle.planar_from_bytes(im, 3), 64, 64)
        X.append(x)
        rows.append(oracle.truth_rows(objs, dx, dy, ratio, 64, 64, ys[0].max_boxes))
    X, rows = np.ascontiguousarray(np.stack(X)), np.stack(rows)
    assert (rows[:, 0, 2:4] > 0).all()                   # boxes with an extent after mapping

    A = dn.HipDarknetTrain(hip, net, params, torch, yolo_loss=True)
    B = dn.HipDarknetTrain(hip, net, params, torch, yolo_loss=True)
    x, truth = A.load_batch(images, boxes)
    hip.finish()
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(X))
    assert np.array_equal(_bits(truth.cpu().numpy()), _bits(rows.reshape(2, -1)))
    A.forward(x, truth=truth)
    B.forward(torch.from_numpy(X).cuda(), truth=torch.from_numpy(rows.reshape(2, -1)).cuda())
    hip.finish()
    for l in ys:
        da, db = A.delta[l.index].cpu().numpy(), B.delta[l.index].cpu().numpy()
        ca, cb = A.costs[l.index].cpu().numpy(), B.costs[l.index].cpu().numpy()
        print("layer", l.index, "cost", ca, "non-zero deltas", int((db != 0).sum()))
        assert (db != 0).any() and cb[0] > 0
        assert np.array_equal(_bits(da), _bits(db)), l.index
        assert np.array_equal(_bits(ca), _bits(cb)), l.index
    assert A.cost() == B.cost() and A.cost() > 0
    with pytest.raises(ValueError, match="box lists"):
        A.load_batch(images, boxes[:1])
