"""tns_region_forward / _loss / _detections against the NumPy restatement of
TRegionLayer (tests/_region_oracle.py), bit for bit."""
import numpy as np
import pytest

from tensorium_amd._abi import TnsError

import _region_oracle as ro

pytestmark = pytest.mark.gpu
F = np.float32
FILL = 7.0   # what an output buffer holds before a call


# forward: h, w, num, classes, batch, softmax, logit spread.  13x13: five whole
# 32-cell tiles and a tail of 9; spread 60: differences where exp rounds to 0
FORWARD = [(1, 1, 1, 1, 1, True, 1), (2, 3, 5, 20, 3, True, 1), (2, 3, 1, 80, 1, False, 1),
           (13, 13, 5, 20, 1, True, 1), (13, 13, 1, 1, 3, False, 1), (13, 13, 5, 80, 1, True, 1),
           (2, 3, 5, 20, 1, True, 60)]


@pytest.mark.parametrize("h, w, num, classes, batch, softmax, spread", FORWARD)
def test_forward_bit_exact(hip, torch_cuda, h, w, num, classes, batch, softmax, spread):
    torch = torch_cuda
    n = batch * num * (classes + 5) * h * w
    x = (np.random.default_rng(n + classes).standard_normal(n) * spread).astype(F)
    want = ro.forward(x, batch, num, classes, h * w, softmax)
    assert spread == 1 or (want.reshape(-1, classes + 5)[:, 5:] == 0).any()  # exp underflowed
    out = torch.full((n,), FILL, device="cuda")
    hip.regionForward(batch, num, classes, h * w, softmax, torch.from_numpy(x).cuda(), out)
    hip.finish()
    ro.same_bits(out, want, "output")


# loss and detections: a 5x4 grid, 3 anchors, 3 classes, batch 2, max=6
G = dict(batch=2, num=3, classes=3, h=4, w=5, biases=(0.8, 1.0, 1.6, 2.2, 3.5, 3.0))


@pytest.fixture(scope="module")
def out5x4():
    x = np.random.default_rng(11).standard_normal(2 * 3 * 8 * 20).astype(F)
    return ro.forward(x, 2, 3, 3, 20, True)


def _truth(*images):
    t = np.zeros((2, 6, 6), F)
    for b, rows in enumerate(images):
        t[b, :len(rows), :5] = rows
    return t


VALID = [(0.11, 0.2, 0.3, 0.4, 0), (0.5, 0.55, 0.2, 0.25, 1), (0.9, 0.9, 0.6, 0.5, 2),
         (0.33, 0.7, 0.15, 0.6, 1), (0.71, 0.3, 0.5, 0.2, 0), (0.45, 0.9, 0.7, 0.7, 2)]
TRUTHS = {
    "empty": _truth(),
    "full": _truth(VALID, VALID[::-1]),                       # no x = 0 terminator
    "bad_class_first": _truth([(0.4, 0.4, 0.3, 0.3, 3)] + VALID[:2], [(0.2, 0.2, 0.5, 0.5, 9)]),
    # class >= classes with x = 0 is skipped, not a break; two truths in cell (2, 2) whose
    # best anchor coincides: the later one stays
    "bad_class_x0": _truth([VALID[0], (0, 0.5, 0.3, 0.3, 7), VALID[2]], [VALID[1]]),
    "same_cell": _truth([(0.5, 0.55, 0.3, 0.5, 1), (0.55, 0.6, 0.32, 0.52, 2)], [VALID[3]]),
    "x_ge_1": _truth([(1.2, 0.5, 0.3, 0.3, 1), VALID[4]], [(0.5, 1.0, 0.2, 0.2, 0)]),
}
LOSS = [(name, {}) for name in TRUTHS] + [
    ("full", dict(seen=12800)), ("full", dict(rescore=True)), ("same_cell", dict(bias_match=True)),
    ("full", dict(classfix=-1)), ("full", dict(classfix=1)), ("full", dict(classfix=2, seen=12800)),
    ("full", dict(thresh=0.6, coord_scale=1.5, object_scale=5, noobject_scale=0.5,
                  class_scale=2))]


@pytest.mark.parametrize("name, over", LOSS)
def test_loss_bit_exact(hip, torch_cuda, out5x4, name, over):
    torch = torch_cuda
    # regionLoss's order; thresh 0.1: cells overlapping a truth take the best-iou branch
    kw = dict(G, max_boxes=6, seen=0, rescore=False, bias_match=False, classfix=0, thresh=0.1,
              coord_scale=1, object_scale=1, noobject_scale=1, class_scale=1) | over
    want_delta, want_cost = ro.loss(out5x4, TRUTHS[name], **kw)
    out = torch.from_numpy(out5x4.copy()).cuda()
    delta, cost = (torch.full((n,), FILL, device="cuda") for n in (out5x4.size, 1))
    hip.regionLoss(*kw.values(), out, torch.from_numpy(TRUTHS[name]).cuda(), delta, cost)
    hip.finish()
    ro.same_bits(delta, want_delta, "delta")
    ro.same_bits(cost, np.array([want_cost]), "cost")
    ro.same_bits(out, out5x4, "output")


DETS = {  # thresh 2: no probability passes; 640x360 letterboxed into 160x128
    "none": dict(thresh=2.0), "some": dict(thresh=0.2), "classfix": dict(thresh=0.2, classfix=-1),
    "letter": dict(thresh=0.2, letter=True, relative=False, im_w=640, im_h=360),
    "capacity": dict(thresh=0.2, capacity=2), "append": dict(thresh=0.2, start=(1, 3))}


@pytest.mark.parametrize("name", sorted(DETS))
def test_detections_bit_exact(hip, torch_cuda, out5x4, name):
    torch = torch_cuda
    kw = dict(G, classfix=0, net_w=160, net_h=128, im_w=160, im_h=128, relative=True,
              letter=False, capacity=70, start=(0, 0)) | DETS[name]
    cap, start, B, classes = kw.pop("capacity"), kw.pop("start"), kw.pop("batch"), kw["classes"]
    want = [ro.detections(out5x4, b, **kw) for b in range(B)]
    taken = [len(w[1]) for w in want]
    assert (max(taken) == 0) == (name == "none") and (name != "capacity" or min(taken) > cap)
    counts = torch.tensor(start, dtype=torch.int64, device="cuda")
    boxes, obj, probs = (torch.full((B, cap, m), FILL, device="cuda") for m in (4, 1, classes))
    hip.regionDetections(B, kw["num"], classes, kw["h"], kw["w"], kw["biases"], kw["classfix"],
                         kw["net_w"], kw["net_h"], kw["im_w"], kw["im_h"], kw["thresh"],
                         kw["relative"], kw["letter"], torch.from_numpy(out5x4).cuda(), cap,
                         counts, boxes, obj, probs)
    hip.finish()
    assert counts.cpu().tolist() == [s + t for s, t in zip(start, taken)]
    for b in range(B):     # the rows that fit stand behind the start; the rest keeps the fill
        m = min(taken[b], cap - start[b])
        for got, w, what in zip((boxes, obj, probs), want[b], ("boxes", "objectness", "probs")):
            g = got[b].cpu().numpy().reshape(cap, -1)
            ro.same_bits(g[start[b]:start[b] + m], w.reshape(taken[b], g.shape[1])[:m], (what, b))
            assert (g[:start[b]] == FILL).all() and (g[start[b] + m:] == FILL).all(), (what, b)


# each TNS_ERR_ARG condition, refused before anything is written
BAD = [("forward", dict(batch=-1)), ("forward", dict(num=100, classes=80)),
       ("forward", dict(inp=None)), ("forward", dict(inp="out")), ("loss", dict(max_boxes=0)),
       ("loss", dict(max_boxes=2049)), ("loss", dict(seen=-1)), ("loss", dict(num=33)),
       ("loss", dict(delta=None)), ("detections", dict(capacity=0)),
       ("detections", dict(net_w=0)), ("detections", dict(im_h=0)),("detections", dict(boxes=None))]


@pytest.mark.parametrize("entry, over", BAD)
def test_argument_guards(hip, torch_cuda, entry, over):
    torch = torch_cuda
    n = 2 * 3 * 8 * 20
    t = {k: torch.full((m,), FILL, device="cuda") for k, m in
         dict(inp=n, out=n, truth=72, delta=n, cost=1, boxes=72, obj=18, probs=54).items()}
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    a = dict(batch=2, num=3, classes=3, max_boxes=6, seen=0, capacity=9, net_w=160, im_h=128, **t)
    a.update({k: a["out"] if v == "out" else v for k, v in over.items()})
    bs = (0.5,) * (2 * a["num"])
    with pytest.raises(TnsError, match="tns status 1"):      # TNS_ERR_ARG
        if entry == "forward":
            hip.regionForward(a["batch"], a["num"], a["classes"], 20, True, a["inp"], a["out"])
        elif entry == "loss":
            hip.regionLoss(2, a["num"], 3, 4, 5, bs, a["max_boxes"], a["seen"], False, False, 0,
                           0.5, 1, 1, 1, 1, a["inp"], a["truth"], a["delta"], a["cost"])
        else:
            hip.regionDetections(2, 3, 3, 4, 5, bs, 0, a["net_w"], 128, 160, a["im_h"], 0.0, True,
                                 False, a["inp"], a["capacity"], counts, a["boxes"], a["obj"],
                                 a["probs"])
    hip.finish()
    assert all((v == FILL).all().item() for v in t.values()) and counts.cpu().tolist() == [0, 0]
