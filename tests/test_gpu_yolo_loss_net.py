"""yolov3-tiny trained end to end with the loss on the device:
HipDarknetTrain(yolo_loss=True) over two iterations of forward(truth) /
backward / update and a third forward.  After each forward every yolo
layer's delta and cost are the oracle's for that layer's device output, and
cost() is their TNNet.cost.  A second driver without the switch runs on the
same inputs with the oracle's deltas handed in through set_yolo_deltas; after
every pass all its weight, update and delta buffers equal the first
driver's bit for bit, which ties the new path to the backward that
tests/test_gpu_train_net.py already verifies."""
import numpy as np
import pytest

from tensorium_amd import darknet as dn

from _yolo_loss_oracle import layer_kwargs, yolo_loss

pytestmark = pytest.mark.gpu
F = np.float32


def _same(a, b, what):
    x, y = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what


def _compare(net, A, B, when):
    for l in net.layers:
        _same(A.delta[l.index], B.delta[l.index], f"{when}: delta {l.index} ({l.kind})")
        _same(A.out[l.index], B.out[l.index], f"{when}: output {l.index} ({l.kind})")
    for i, st in A.conv.items():
        for k, v in st.items():
            _same(v, B.conv[i][k], f"{when}: conv {i} {k}")


def test_yolov3_tiny_trains_with_the_device_loss(hip, torch_cuda):
    torch = torch_cuda
    net = dn.Network(dn.parse_cfg(dn.yolov3_tiny_cfg(64, batch=2, classes=3)))
    ys = [l for l in net.layers if l.kind == "yolo"]
    assert [(l.h, l.w) for l in ys] == [(2, 2), (4, 4)]
    params = dn.random_params(net, seed=71)
    rng = np.random.default_rng(72)
    x = torch.from_numpy(rng.standard_normal((2, 3 * 64 * 64)).astype(F)).cuda()
    truth = np.zeros((2, 200, 6), dtype=F)
    # image 0: a large and a small box and one of an invalid class between
    # them; image 1: two boxes in the same cell of the coarse grid
    truth[0, :3] = [(0.3, 0.6, 0.9, 0.8, 1, 1), (0.5, 0.5, 0.3, 0.3, 7, 2),
                    (0.8, 0.2, 0.2, 0.3, 2, 3)]
    truth[1, :2] = [(0.7, 0.7, 0.5, 0.6, 0, 4), (0.8, 0.8, 0.55, 0.5, 2, 5)]
    T = torch.from_numpy(truth.reshape(2, -1)).cuda()
    A = dn.HipDarknetTrain(hip, net, params, torch, yolo_loss=True)
    B = dn.HipDarknetTrain(hip, net, params, torch)
    with pytest.raises(ValueError, match="no loss layer"):
        B.cost()
    writes = 0
    for it in range(3):
        A.forward(x, truth=T)
        hip.finish()
        want = []
        for l in ys:
            r = yolo_loss(A.out[l.index].cpu().numpy(), truth, **layer_kwargs(l, net))
            writes += r["counters"]["truth_writes"]
            delta, cost = A.delta[l.index].cpu().numpy(), A.costs[l.index].cpu().numpy()
            print("iteration", it, "layer", l.index, "cost", cost[0], "oracle", r["cost"])
            assert np.array_equal(delta.view(np.uint32), r["delta"].view(np.uint32)), (it, l.index)
            assert cost.view(np.uint32)[0] == np.asarray(r["cost"]).view(np.uint32), (it, l.index)
            want.append(r)
        s = F(0)
        for r in want:                      # TNNet.cost: the sum over the count, singles
            s = F(s + r["cost"])
        assert A.cost() == float(F(s / F(len(want))))
        B.forward(x)
        B.set_yolo_deltas([torch.from_numpy(r["delta"]).cuda() for r in want])
        hip.finish()
        _compare(net, A, B, f"forward {it}")
        if it == 2:
            break
        A.backward(x)
        B.backward(x)
        hip.finish()
        _compare(net, A, B, f"backward {it}")
        A.update(0.001, 0.9, 0.0005)
        B.update(0.001, 0.9, 0.0005)
        hip.finish()
        _compare(net, A, B, f"update {it}")
    assert writes > 0                        # the truths reached both layers' truth pass
    assert A.yolo_counters.cpu().tolist()[0] > 0
