"""HipDarknet.detections on yolov3-tiny: forward, then the detections with and
without NMS against the oracle run on the device's own yolo outputs copied
back, bit for bit, so that the test pins the detection path and not the
convolutions.  thresh is a quantile of those outputs' objectness values, so
that a few dozen rows an image pass whatever the random parameters give."""
import numpy as np
import pytest

from tensorium_amd import darknet as dn
from tensorium_amd._abi import TnsError

import _detections_oracle as oracle

pytestmark = pytest.mark.gpu
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _oracle_rows(net, ys, outs, b, thresh, im, relative, letter, counters):
    parts = [oracle.get_detections(o, b, n=l.anchors, classes=l.classes, h=l.h, w=l.w,
                                   mask=l.mask, biases=l.biases, net_w=net.w, net_h=net.h,
                                   im_w=im[0], im_h=im[1], thresh=thresh, relative=relative,
                                   letter=letter, counters=counters)
             for l, o in zip(ys, outs)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def test_yolov3_tiny_detections(hip, torch_cuda):
    torch = torch_cuda
    net = dn.Network(dn.parse_cfg(dn.yolov3_tiny_cfg(size=96, batch=2, classes=3)))
    ys = [l for l in net.layers if l.kind == "yolo"]
    assert [(l.h, l.w) for l in ys] == [(3, 3), (6, 6)]
    params = dn.random_params(net, seed=81)
    rng = np.random.default_rng(82)
    x = torch.from_numpy(rng.standard_normal((2, 3 * 96 * 96)).astype(F)).cuda()

    def yolo_outputs(ps):
        A = dn.HipDarknet(hip, net, ps, torch)
        A.forward(x)
        hip.finish()
        return A, [A.out[l.index].cpu().numpy() for l in ys]

    def objectness(outs):
        return np.concatenate([o.reshape(2, l.anchors, l.classes + 5, -1)[:, :, 4].reshape(-1)
                               for l, o in zip(ys, outs)])

    # random_params leaves every logistic output near 0.5, where no objectness
    # * class product passes a thresh that objectness values pass.  The two
    # head convolutions (linear, no batch norm) are scaled so that the
    # objectness logits have a standard deviation of 2
    _, outs = yolo_outputs(params)
    o = objectness(outs).astype(np.float64)
    gain = F(2.0 / np.std(np.log(o / (1 - o))))
    for p, l in zip(params, net.param_layers()):
        if net.layers[l.index + 1].kind == "yolo":
            p.weights *= gain
            p.biases *= gain
    A, outs = yolo_outputs(params)
    thresh = float(F(np.quantile(objectness(outs), 0.6)))   # 270 candidates: about 54 an image
    im = (640, 427)
    scores = 0
    for relative, letter, nms in ((False, True, None), (True, False, 0.45), (False, True, 0.45)):
        c = oracle.new_counters()
        got = A.detections(im[0], im[1], thresh=thresh, relative=relative, letter=letter, nms=nms)
        assert len(got) == 2
        for b, (boxes, obj, probs) in enumerate(got):
            wb, wo, wp = _oracle_rows(net, ys, outs, b, thresh, im, relative, letter, c)
            if nms is not None:
                scores += int((wp != 0).sum())
                wp = oracle.nms_sort(wb, wo, wp, nms, counters=c)
            print("image", b, "rows", wo.size, "non-zero scores", int((wp != 0).sum()))
            assert boxes.shape == wb.shape and probs.shape == wp.shape
            assert np.array_equal(_bits(obj), _bits(wo)), (b, "objectness / row order")
            assert np.array_equal(_bits(boxes), _bits(wb)), (b, "boxes")
            assert np.array_equal(_bits(probs), _bits(wp)), (b, "probs")
        print("thresh", thresh, "nms", nms, c)
        assert 60 <= c["taken"] <= 160, c             # a few dozen rows an image
    assert scores > 0                                 # NMS had scores to work on
    # the same rows again through an explicit capacity that holds them ...
    most = max(g[1].size for g in got)
    again = A.detections(im[0], im[1], thresh=thresh, relative=False, letter=True, nms=0.45,
                         capacity=most)
    for g, a in zip(got, again):
        assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(g, a))
    # ... and one that does not: the image and its count are named
    with pytest.raises(TnsError, match=r"image \d+ has \d+ taken candidates, capacity 5"):
        A.detections(im[0], im[1], thresh=thresh, capacity=5)


def test_heads_that_disagree_on_classes_are_refused(hip, torch_cuda):
    head, tail = dn.yolov3_tiny_cfg(size=96, batch=2, classes=3).rsplit("[yolo]", 1)
    tail = tail.replace("mask = 0,1,2", "mask = 0,1").replace("classes=3", "classes=7")
    net = dn.Network(dn.parse_cfg(head + "[yolo]" + tail))
    ys = [l for l in net.layers if l.kind == "yolo"]
    assert [(l.anchors, l.classes) for l in ys] == [(3, 3), (2, 7)]
    A = dn.HipDarknet(hip, net, dn.random_params(net, seed=83), torch_cuda)
    A.forward(torch_cuda.zeros(2, 3 * 96 * 96, device="cuda"))
    with pytest.raises(ValueError, match="disagree on classes"):
        A.detections(640, 427)
