"""tns_hip_yolo_loss against the NumPy restatement of TYoloLayer.forward's
training part, bit for bit: delta, cost, the output after the call (the
NaN / Inf objectness reset), the per-image stats and the two counters.  The
cases and what each one must reach: tests/_yolo_loss_cases.py; that they do
reach it is asserted here too, from the oracle's counters, before the device
result is looked at."""
import numpy as np
import pytest

from tensorium_amd._abi import TnsError

import _yolo_loss_cases as cases
from _yolo_loss_oracle import COUNTERS

pytestmark = pytest.mark.gpu

FILL = 7.0   # what delta holds before a call: the call overwrites every element


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _call(hip, torch, out_np, truth_np, kw, **over):
    B = kw["batch"]
    buf = dict(output=torch.from_numpy(np.array(out_np)).cuda(),
               truth=torch.from_numpy(np.array(truth_np)).cuda(),
               delta=torch.full((out_np.size,), FILL, device="cuda"),
               cost=torch.full((1,), FILL, device="cuda"),
               stats=torch.full((2 * B,), FILL, device="cuda"),
               counters=torch.tensor([5, 3], dtype=torch.int64, device="cuda"))
    a = dict(kw, **buf)
    a.update(over)
    hip.yoloLoss(a["batch"], a["n"], a["classes"], a["h"], a["w"], a["total"], a["mask"],
                 a["biases"], a["max_boxes"], a["net_w"], a["net_h"], a["ignore_thresh"],
                 a["truth_thresh"], a["iou_thresh"], a["iou_normalizer"], a["obj_normalizer"],
                 a["output"], a["truth"], a["delta"], a["cost"], a["stats"], a["counters"])
    hip.finish()
    return buf


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_yolo_loss_bit_exact(hip, torch_cuda, name):
    out, truth, kw = cases.build(name)
    want = cases.expected(name)
    for need in cases.CASES[name]["needs"]:      # a case that misses its branch fails
        assert want["counters"][need] > 0, (name, need, want["counters"])
    got = _call(hip, torch_cuda, out, truth, kw)
    delta = got["delta"].cpu().numpy()
    bad = np.flatnonzero(_bits(delta) != _bits(want["delta"]))
    assert bad.size == 0, (name, bad[:8], delta[bad[:8]], want["delta"][bad[:8]])
    cost = got["cost"].cpu().numpy()
    print(name, "cost", cost[0], "oracle", want["cost"])
    assert _bits(cost)[0] == _bits(want["cost"]), (cost[0], want["cost"])
    assert np.array_equal(_bits(got["output"].cpu().numpy()), _bits(want["output"]))
    assert np.array_equal(_bits(got["stats"].cpu().numpy()), _bits(want["stats"].reshape(-1)))
    # the counters are added to what the buffer held
    assert got["counters"].cpu().tolist() == [5 + want["total_bbox"], 3 + want["rewritten_bbox"]]


def test_every_counter_reached_somewhere():
    for k in COUNTERS + ("unmatched",):
        assert any(cases.expected(n)["counters"][k] > 0 for n in cases.CASES), k


def test_stats_are_optional(hip, torch_cuda):
    out, truth, kw = cases.build("3x5_lists")
    got = _call(hip, torch_cuda, out, truth, kw, stats=None)
    assert np.array_equal(_bits(got["delta"].cpu().numpy()),
                          _bits(cases.expected("3x5_lists")["delta"]))


@pytest.mark.parametrize("over", [
    dict(batch=-1), dict(classes=-1), dict(h=-1), dict(w=-1), dict(net_w=0), dict(net_h=-4),
    dict(max_boxes=0), dict(max_boxes=-2), dict(mask=(0, 1, 6)), dict(mask=(0, -1, 2)),
    dict(output=None), dict(truth=None), dict(delta=None), dict(cost=None), dict(counters=None)],
    ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_argument_guards(hip, torch_cuda, over):
    out, truth, kw = cases.build("3x5_full_list")
    torch = torch_cuda
    delta = torch.full((out.size,), FILL, device="cuda")
    with pytest.raises(TnsError, match="tns status 1"):      # TNS_ERR_ARG
        _call(hip, torch, out, truth, kw, **dict(dict(delta=delta), **over))
    hip.finish()
    assert (delta == FILL).all().item()
