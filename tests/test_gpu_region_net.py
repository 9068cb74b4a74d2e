"""Three convolutions and a maxpool into [region], 32x32, batch 2, through the
public drivers: output, detections after NMS, delta and cost are the oracle's,
and a second driver handed the oracle's delta ends with the same weights."""
import numpy as np
import pytest

from tensorium_amd import darknet as dn

import _region_oracle as ro
from _detections_oracle import nms_sort

pytestmark = pytest.mark.gpu
F = np.float32


def _conv(f, k, s, bn):
    return (f"[convolutional]\nbatch_normalize={bn}\nfilters={f}\nsize={k}\nstride={s}\npad=1\n"
            f"activation={'leaky' if bn else 'linear'}\n")


CFG = ("[net]\nbatch=2\nheight=32\nwidth=32\nchannels=3\n" + _conv(8, 3, 1, 1)
       + "[maxpool]\nsize=2\nstride=2\n" + _conv(16, 3, 2, 1) + _conv(16, 1, 1, 0)
       + "[region]\nanchors=1.5,2.0, 4.0,3.0\nnum=2\nclasses=3\nsoftmax=1\nrescore=1\n"
         "bias_match=1\nmax=4\nthresh=.3\nobject_scale=5\n")


def _kw(l, **more):
    return dict(num=l.anchors, classes=l.classes, h=l.h, w=l.w, biases=l.biases, **more)


def test_region_net_detects_and_trains(hip, torch_cuda):
    torch = torch_cuda
    net = dn.Network(dn.parse_cfg(CFG))
    l = net.layers[-1]
    params = dn.random_params(net, seed=5)
    x = torch.from_numpy(np.random.default_rng(6).standard_normal((2, 3, 32, 32)).astype(F)).cuda()

    inf = dn.HipDarknet(hip, net, params, torch)
    out = inf.forward(x)
    hip.finish()
    region = ro.forward(out[l.index - 1].cpu().numpy(), 2, l.anchors, l.classes, l.h * l.w, True)
    ro.same_bits(out[l.index], region, "region output")
    got = inf.detections(48, 32, thresh=0.2, letter=True, nms=0.45)
    for b in range(2):
        boxes, obj, probs = ro.detections(region, b, **_kw(
            l, classfix=0, net_w=32, net_h=32, im_w=48, im_h=32, thresh=0.2, relative=False,
            letter=True))
        assert len(obj) > 0
        for g, w, what in zip(got[b], (boxes, obj, nms_sort(boxes, obj, probs, 0.45)),
                              ("boxes", "objectness", "probs")):
            ro.same_bits(g, w, (what, b))

    truth = np.zeros((2, 4, 6), F)
    truth[0, :2] = [(0.3, 0.6, 0.4, 0.5, 1, 0), (0.7, 0.2, 0.2, 0.3, 2, 0)]
    truth[1, :1] = [(0.55, 0.5, 0.6, 0.3, 0, 0)]
    T = torch.from_numpy(truth.reshape(2, -1)).cuda()
    A = dn.HipDarknetTrain(hip, net, params, torch)
    B = dn.HipDarknetTrain(hip, net, params, torch)
    A.forward(x, truth=T)
    B.forward(x)
    hip.finish()
    delta, cost = ro.loss(A.out[l.index].cpu().numpy(), truth, batch=2, seen=0, **_kw(
        l, max_boxes=4, rescore=True, bias_match=True, classfix=0, thresh=l.thresh,
        coord_scale=1, object_scale=5, noobject_scale=1, class_scale=1))
    ro.same_bits(A.delta[l.index], delta, "region delta")
    ro.same_bits(A.costs[l.index], np.array([cost]), "region cost")
    assert A.cost() == float(cost)
    B.delta[l.index].copy_(torch.from_numpy(delta).cuda())
    for d in (A, B):
        d.backward(x)
        d.update(0.001, 0.9, 0.0005)
    hip.finish()
    assert A.seen == 2 and any(st["wu"].abs().sum().item() > 0 for st in A.conv.values())
    for i, st in A.conv.items():
        for k, v in st.items():
            ro.same_bits(v, B.conv[i][k], f"conv {i} {k}")
