"""tns_hip_yolo_detections / tns_hip_nms_sort against the NumPy restatement of
getDetections + correctBoxes and doNMSSort, bit for bit: the per-image counts,
the rows' order, boxes, objectness and probs.  Every output buffer is filled
with a sentinel first, so that what must not be written is checked too.  The
cases and what each one must reach: tests/_detections_cases.py (proved on the
CPU in tests/test_detections.py, and asserted here again before the device
result is looked at)."""
import numpy as np
import pytest

from tensorium_amd._abi import TnsError

import _detections_cases as cases

pytestmark = pytest.mark.gpu

F = np.float32
FILL = -7.0     # no row of any case holds it


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(got, want, what):
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
    assert bad.size == 0, (what, bad[:8], np.asarray(got).reshape(-1)[bad[:8]],
                           np.asarray(want).reshape(-1)[bad[:8]])


def _buffers(torch, batch, cap, classes, counts=None):
    return dict(counts=torch.tensor(counts or [0] * batch, dtype=torch.int64, device="cuda"),
                boxes=torch.full((batch, cap, 4), FILL, device="cuda"),
                objectness=torch.full((batch, cap), FILL, device="cuda"),
                probs=torch.full((batch, cap, max(classes, 1)), FILL, device="cuda"))


def _collect(hip, torch, spec, cap, buf, geo, out, **over):
    a = dict(geo, batch=spec["batch"], net_w=spec["net"][0], net_h=spec["net"][1],
             im_w=spec["im"][0], im_h=spec["im"][1], thresh=spec["thresh"],
             relative=spec["relative"], letter=spec["letter"], capacity=cap,
             output=torch.from_numpy(np.array(out)).cuda().reshape(-1), **buf)
    a.update(over)
    hip.yoloDetections(a["batch"], a["n"], a["classes"], a["h"], a["w"], a["total"], a["mask"],
                       a["biases"], a["net_w"], a["net_h"], a["im_w"], a["im_h"], a["thresh"],
                       a["relative"], a["letter"], a["output"], a["capacity"], a["counts"],
                       a["boxes"], a["objectness"], a["probs"])


def _check_rows(buf, want, cap, nms):
    """Counts, then per image the written rows and the sentinel behind them."""
    counts = buf["counts"].cpu().tolist()
    assert counts == [img["count"] for img in want["images"]]
    boxes, obj, probs = (buf[k].cpu().numpy() for k in ("boxes", "objectness", "probs"))
    for b, img in enumerate(want["images"]):
        m = min(img["count"], cap)
        _same(obj[b, :m], img["obj"][:m], ("objectness", b))        # the rows' order
        _same(boxes[b, :m], img["boxes"][:m], ("boxes", b))
        _same(probs[b, :m], img["probs_nms"] if nms else img["probs"][:m], ("probs", b))
        for name, a in (("boxes", boxes), ("objectness", obj), ("probs", probs)):
            assert (a[b, m:] == F(FILL)).all(), (name, b, "written beyond the rows")


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_detections_bit_exact(hip, torch_cuda, name):
    spec, want = cases.build(name), cases.expected(name)
    for need in spec["needs"]:                       # a case that misses its point fails
        assert want["counters"][need] > 0, (name, need, want["counters"])
    assert want["counters"]["ties"] == 0 and want["counters"]["near_thresh"] == 0
    cap, classes = want["capacity"], spec["layers"][0][0]["classes"]
    buf = _buffers(torch_cuda, spec["batch"], cap, classes)
    so_far = [0] * spec["batch"]
    for k, (geo, out) in enumerate(spec["layers"]):  # layers append through counts
        _collect(hip, torch_cuda, spec, cap, buf, geo, out)
        hip.finish()
        so_far = [s + img["layer_counts"][k] for s, img in zip(so_far, want["images"])]
        assert buf["counts"].cpu().tolist() == so_far
    _check_rows(buf, want, cap, nms=False)
    if spec["nms"] is not None:
        hip.nmsSort(spec["batch"], cap, classes, buf["counts"], buf["boxes"], buf["objectness"],
                    buf["probs"], spec["nms"])
        hip.finish()
        _check_rows(buf, want, cap, nms=True)        # boxes, objectness, sentinel untouched


def test_on_chip_limit_is_crossed():
    """kNmsLds = 2048 (csrc/detections.hip) non-zero scores of one (image,
    class) are sorted in LDS; nms_52x52's class 0 has more and takes the
    selection form, its class 1 fewer, in the same launch."""
    probs = cases.expected("nms_52x52")["images"][0]["probs"]
    nonzero = (probs != 0).sum(axis=0)
    assert nonzero[0] > cases.NMS_ON_CHIP > nonzero[1] > 0


def test_nms_leaves_zero_objectness_rows_out(hip, torch_cuda):
    torch = torch_cuda
    boxes, obj, probs, after, c = cases.zero_objectness_rows()
    assert c["zero_obj"] > 3 and c["suppressed"] > 0 and c["ties"] == 0 and c["near_thresh"] == 0
    m, classes = obj.size, probs.shape[1]
    cap = m + 5
    buf = _buffers(torch, 1, cap, classes, counts=[m])
    buf["boxes"][0, :m] = torch.from_numpy(boxes).cuda()
    buf["objectness"][0, :m] = torch.from_numpy(obj).cuda()
    buf["probs"][0, :m] = torch.from_numpy(probs).cuda()
    hip.nmsSort(1, cap, classes, buf["counts"], buf["boxes"], buf["objectness"], buf["probs"],
                cases.NMS)
    hip.finish()
    _same(buf["probs"][0, :m].cpu().numpy(), after, "probs")
    assert (buf["probs"][0, m:] == FILL).all().item()
    _same(buf["boxes"][0, :m].cpu().numpy(), boxes, "boxes")
    _same(buf["objectness"][0, :m].cpu().numpy(), obj, "objectness")
    assert buf["counts"].cpu().tolist() == [m]


def _untouched(buf, counts):
    assert buf["counts"].cpu().tolist() == counts
    for k in ("boxes", "objectness", "probs"):
        assert (buf[k] == FILL).all().item(), k


@pytest.mark.parametrize("over", [
    dict(batch=-1), dict(classes=-1), dict(h=-1), dict(w=-1), dict(net_w=0), dict(net_h=-4), dict(im_w=0), dict(im_h=-1), dict(mask=(3, 4, 6)),
    dict(mask=(3, -1, 5)), dict(n=33, mask=tuple(range(33)), total=33, biases=(1.0,) * 66),
    dict(total=33, biases=(1.0,) * 66), dict(capacity=0), dict(capacity=-3),
    dict(capacity=(1 << 22) + 1), dict(batch=70000), dict(classes=1 << 29),
    dict(capacity=1 << 22, classes=1 << 10), dict(output=None), dict(counts=None),
    dict(boxes=None), dict(objectness=None), dict(probs=None)],
    ids=lambda o: "-".join(f"{k}={v if not isinstance(v, tuple) else len(v)}"
                           for k, v in o.items()))
def test_collect_argument_guards(hip, torch_cuda, over):
    spec = cases.build("3x5_b3")
    geo, out = spec["layers"][0]
    buf = _buffers(torch_cuda, 3, 45, 4, counts=[2, 0, 1])
    with pytest.raises(TnsError, match="tns status 1"):      # TNS_ERR_ARG
        _collect(hip, torch_cuda, spec, 45, buf, geo, out, **over)
    hip.finish()
    _untouched(buf, [2, 0, 1])


@pytest.mark.parametrize("anchors,total", [(-1, 6), (3, -1)])
def test_collect_negative_anchor_counts(hip, torch_cuda, anchors, total):
    """(TNNHip.yoloDetections sizes mask and biases by these two, so a
    negative one reaches the library only from a direct call)"""
    import ctypes as C
    torch = torch_cuda
    buf = _buffers(torch, 3, 45, 4, counts=[2, 0, 1])
    out = torch.zeros(3 * 3 * 9 * 15, device="cuda")
    mask, biases = (C.c_int64 * 3)(3, 4, 5), (C.c_float * 12)(*cases.ANCHORS)
    rc = hip.lib.tns_hip_yolo_detections(
        hip.ctx, 3, anchors, 4, 3, 5, total, mask, biases, 160, 96, 517, 389, 0.25, 0, 0,
        out.data_ptr(), 45, buf["counts"].data_ptr(), buf["boxes"].data_ptr(),
        buf["objectness"].data_ptr(), buf["probs"].data_ptr())
    hip.lib.tns_clear_error()
    assert rc == 1                                           # TNS_ERR_ARG
    hip.finish()
    _untouched(buf, [2, 0, 1])


@pytest.mark.parametrize("over", [
    dict(batch=-1), dict(classes=-1), dict(capacity=0), dict(capacity=-1),
    dict(capacity=(1 << 22) + 1), dict(batch=70000), dict(capacity=1 << 22, classes=1 << 10),
    dict(counts=None), dict(boxes=None), dict(objectness=None), dict(probs=None)],
    ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_nms_argument_guards(hip, torch_cuda, over):
    buf = _buffers(torch_cuda, 2, 9, 4, counts=[9, 9])
    a = dict(buf, batch=2, capacity=9, classes=4)
    a.update(over)
    with pytest.raises(TnsError, match="tns status 1"):
        hip.nmsSort(a["batch"], a["capacity"], a["classes"], a["counts"], a["boxes"],
                    a["objectness"], a["probs"], 0.45)
    hip.finish()
    _untouched(buf, [9, 9])


def test_empty_calls_succeed(hip, torch_cuda):
    spec = cases.build("3x5_b3")
    geo, out = spec["layers"][0]
    buf = _buffers(torch_cuda, 3, 45, 4)
    _collect(hip, torch_cuda, spec, 45, buf, geo, out, batch=0)
    _collect(hip, torch_cuda, spec, 45, buf, geo, out, batch=0, output=None, counts=None,
             boxes=None, objectness=None, probs=None)
    hip.nmsSort(0, 45, 4, None, None, None, None, 0.45)
    hip.nmsSort(3, 45, 4, buf["counts"], buf["boxes"], buf["objectness"], buf["probs"], 0.45)
    hip.finish()                                     # all counts zero: nothing read or written
    _untouched(buf, [0, 0, 0])
