"""The fused connected-network train step (mlp_train.hip) off the MNIST
shapes: the 5-slots-per-thread kernel instance, the late weight-update pass,
channels past thread 1023, odd batch x width, the LDS-staged forward gemm's
scalar and two-batch-tile forms, misaligned operands, the layer-0 forward's
chunk boundaries, 1 and 16 layers, one class, the delta clamp, the loss floor,
a dead batch-norm channel and the argument checks.

Bar: bit-exact against the oracle (cost and every buffer element), as in
test_gpu_train.py.  The device buffer sits between two runs of guard floats,
so a store past a layer's arrays is seen."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = np.float32(-77.25)
HYPER = (1e-2, 0.9, 1e-4)  # lr, momentum, decay


def guarded(T, host, shift=0):
    """host copied into a view of a larger sentinel-filled device tensor:
    GUARD floats either side, the view `shift` floats past a 16-byte boundary."""
    n = host.size
    whole = T.full((GUARD + shift + n + GUARD,), float(SENT), device="cuda")
    view = whole[GUARD + shift:GUARD + shift + n]
    view.copy_(T.from_numpy(host.copy()))  # (the shared reference arrays are read-only)
    assert view.data_ptr() % 16 == 4 * shift
    return whole, view


def guards_intact(whole, shift, n):
    w = whole.cpu().numpy()
    return bool(np.all(w[:GUARD + shift] == SENT) and np.all(w[GUARD + shift + n:] == SENT))


_REF = {}


def reference(ora, widths, acts, B, bn, steps, hyper=HYPER, prep=None):
    """Oracle run, once per configuration: X, truth, the initial buffer and
    (cost, buffer) after each of `steps` steps.  Shared: read only."""
    key = (tuple(widths), tuple(acts), B, bn, steps, hyper, prep.__name__ if prep else None)
    if key not in _REF:
        buf = ora.mlp_init(widths, bn, B, seed=11)
        if prep:
            prep(widths, bn, B, buf)
        X, truth = ora.mnist_batch(B, seed=11, classes=widths[-1], inputs=widths[0])
        buf0 = buf.copy()
        after = []
        for _ in range(steps):
            cost = ora.mlp_train_step(widths, acts, bn, B, X, truth, *hyper, buf)
            after.append((np.float32(cost), buf.copy()))
        for a in (X, truth, buf0, *[b for _, b in after]):
            a.setflags(write=False)
        _REF[key] = (X, truth, buf0, after)
    return _REF[key]


def check_steps(hip, T, ora, widths, acts, B, bn, steps=3, hyper=HYPER, prep=None, shift=0,
                check_after=None):
    X, truth, buf0, after = reference(ora, widths, acts, B, bn, steps, hyper, prep)
    whole, dbuf = guarded(T, buf0, shift)
    _, dX = guarded(T, X, shift)
    dT = T.from_numpy(truth.copy()).cuda()
    dcost = T.zeros(1, device="cuda")
    for s in range(steps):
        hip.mlpTrainStep(widths, acts, bn, B, dX, dT, *hyper, dbuf, dcost)
        if s + 1 in (check_after or (steps,)):
            hip.finish()
            cost, ref = after[s]
            assert np.all(np.isfinite(ref)) and np.isfinite(cost)
            got = dbuf.cpu().numpy()
            assert np.float32(dcost.item()) == cost, (s + 1, float(dcost.item()), float(cost))
            diff = np.flatnonzero(got != ref)
            assert diff.size == 0, (s + 1, diff.size, diff[:10])
    assert guards_intact(whole, shift, buf0.size), "wrote outside the packed buffer"
    assert not np.array_equal(after[-1][1], buf0)  # (the step moved the buffer)


SHAPES = [
    # the 5-slot instance (B*O = 4096); layer 1 has 4*4 + 1*4 = 20 tiles: the
    # late update pass, more than one dW/dX task per wave
    ([200, 128, 128, 10], [1, 9, 4], 32),
    # 5-slot instance; every layer updates in its dW waves (1*4 + 1*4 tiles)
    # next to the net above, where layer 1 does not
    ([96, 128, 32, 10], [1, 1, 4], 32),
    # LDS-staged gemm with two batch tiles; hand-off block after the chunks
    ([64, 32, 32, 10], [1, 8, 4], 48),
    # LDS-staged gemm, scalar staging (odd I)
    ([50, 37, 30, 10], [9, 1, 4], 20),
    # channels past thread 1023; 5-slot instance
    ([40, 1100, 10], [1, 4], 4),
    # the LDS limit exactly (9*3*1517 = 40959); one layer; odd B*O; O > 1024
    ([9, 1517], [4], 3),
    # one layer; widest O at batch 2
    ([12, 2275], [4], 2),
    # odd B*O: scalar copy of layer 0's partials; tiny tiles
    ([7, 5, 3], [1, 4], 3),
    # one layer; odd batch; odd input width
    ([33, 10], [4], 7),
    # odd batch across two batch tiles; odd B*O in layer 0; 5-slot instance
    ([64, 63, 64, 10], [1, 1, 4], 33),
    # last input width of the register-resident layer-0 forward
    ([1024, 8, 10], [1, 4], 4),
    # first width past it: 9 chunks, two in flight
    ([1028, 8, 10], [1, 4], 4),
    # 16 layers
    ([20] + [16] * 15 + [10], [1] * 15 + [4], 8),
    # one class: the cost is exactly 0, the buffers still move
    ([30, 20, 1], [1, 4], 5),
]


@pytest.mark.parametrize("bn", [0, 1])
@pytest.mark.parametrize("widths,acts,B", SHAPES,
                         ids=[("x".join(map(str, w)) if len(w) < 6 else f"{len(a)}layers") + f"-b{B}"
                              for w, a, B in SHAPES])
def test_fused_mlp_off_mnist_shapes(hip, torch_cuda, ora, widths, acts, B, bn):
    """Cost and every buffer element bit-identical to the oracle after 3
    steps, guards untouched."""
    assert 9 * B * max(widths[1:]) <= 40960
    check_steps(hip, torch_cuda, ora, widths, acts, B, bn)
    if widths[-1] == 1:
        assert reference(ora, widths, acts, B, bn, 3)[3][-1][0] == 0.0


@pytest.mark.parametrize("shift", [1, 2])
@pytest.mark.parametrize("bn", [0, 1])
def test_fused_mlp_misaligned_operands(hip, torch_cuda, ora, bn, shift):
    """buf and X 4 and 8 bytes past a 16-byte boundary: every input width is
    a multiple of 4 and every pointer test of the float4 paths is false.  Same
    result as the aligned run (the oracle's)."""
    check_steps(hip, torch_cuda, ora, [64, 32, 32, 10], [1, 1, 4], 16, bn, shift=shift)


@pytest.mark.parametrize("hyper", [(0.05, 0.0, 0.0), (1e-2, 0.5, 1e-2)],
                         ids=["lr.05-mom0-decay0", "mom.5-decay.01"])
@pytest.mark.parametrize("bn", [0, 1])
def test_fused_mlp_hyperparameters(hip, torch_cuda, ora, bn, hyper):
    """(learning rate, momentum, decay) other than the 1e-2 / 0.9 / 1e-4 of every
    other case, on the net whose layer 1 takes the late update pass."""
    check_steps(hip, torch_cuda, ora, [200, 128, 128, 10], [1, 9, 4], 32, bn, hyper=hyper)


CLAMP_NET = ([64, 64, 64, 10], [1, 1, 4], 32)


def layer_offsets(widths, bn, B):
    """element offset of each layer's arrays in the packed buffer"""
    offs, p = [], 0
    for l in range(len(widths) - 1):
        I, O = widths[l], widths[l + 1]
        names = [("W", I * O), ("b", O), ("dW", I * O), ("db", O)]
        if bn:
            names += [(k, O) for k in ("scales", "rmean", "rvar", "dscales")]
        names += [("out", B * O), ("delta", B * O)]
        if bn:
            names += [("x", B * O), ("xnorm", B * O)] + [(k, O) for k in
                                                         ("mean", "var", "mdelta", "vdelta")]
        d = {}
        for k, n in names:
            d[k] = (p, n)
            p += n
        offs.append(d)
    return offs


def weights_times_4(widths, bn, B, buf):
    for l, d in enumerate(layer_offsets(widths, bn, B)):
        p, n = d["W"]
        buf[p:p + n] *= np.float32(4)


def dead_channel(widths, bn, B, buf):
    p, _ = layer_offsets(widths, bn, B)[0]["W"]
    buf[p:p + widths[0]] = 0.0  # row 0 of layer 0's W: channel 0 is 0 in every row of the batch


def test_fused_mlp_clamp_and_loss_floor(hip, torch_cuda, ora):
    """Weights x 4: delta.Clamp(-1, 1) clamps in layers 1 and 0 and some
    true-class probabilities sit below the loss's floor.  Both are recounted
    here in float64 so that the case cannot pass without reaching them."""
    widths, acts, B = CLAMP_NET
    X, truth, buf0, _ = reference(ora, widths, acts, B, 0, 3, prep=weights_times_4)
    offs = layer_offsets(widths, 0, B)
    Ws = [buf0[d["W"][0]:d["W"][0] + d["W"][1]].astype(np.float64).reshape(widths[l + 1], widths[l])
          for l, d in enumerate(offs)]
    x = X.astype(np.float64).reshape(B, widths[0])
    outs = []
    for l, W in enumerate(Ws):  # (biases are 0 at the start)
        x = x @ W.T
        if acts[l] == 1:
            x = x * (x > 0)
        outs.append(x)
    e = np.exp(x - x.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    t = truth.astype(np.float64).reshape(B, -1)
    floored = int(np.sum(p[t != 0] <= 1e-6))
    delta = t - p
    clamped = {}
    for l in (2, 1):
        delta = np.clip(delta, -1, 1)
        if acts[l] == 1:
            delta = delta * (outs[l] > 0)
        delta = delta @ Ws[l]
        clamped[l - 1] = float(np.mean(np.abs(delta) > 1))
    print(f"true-class p <= 1e-6: {floored} of {B}; |delta| > 1 before the clamp: {clamped}")
    assert floored > 0 and clamped[1] > 0 and clamped[0] > 0
    check_steps(hip, torch_cuda, ora, widths, acts, B, 0, prep=weights_times_4,
                check_after=(1, 3))


def test_fused_mlp_dead_bn_channel(hip, torch_cuda, ora):
    """A channel whose variance is exactly 0: the var <= eps sides of the
    forward normalize and of mean_delta / variance_delta (pow(eps, -1.5))."""
    widths, acts, B = CLAMP_NET
    _, _, _, after = reference(ora, widths, acts, B, 1, 3, prep=dead_channel)
    p, _ = layer_offsets(widths, 1, B)[0]["var"]
    for _, buf in after:
        assert buf[p] == 0.0 and np.all(buf[p + 1:p + widths[1]] > 0.0)
    check_steps(hip, torch_cuda, ora, widths, acts, B, 1, prep=dead_channel, check_after=(1, 3))


ERR_ARG, ERR_UNSUPPORTED = 1, 4  # TNS_ERR_ARG, TNS_ERR_UNSUPPORTED (include/tns.h)


def test_fused_mlp_argument_errors(hip, torch_cuda):
    """Bad arguments are error codes, and neither buf nor cost is written."""
    L, T = hip.lib, torch_cuda
    n = 60000
    buf = T.full((n,), float(SENT), device="cuda")
    cost = T.full((1,), float(SENT), device="cuda")
    X = T.zeros(4096, device="cuda")
    truth = T.zeros(8192, device="cuda")

    def call(widths, acts, B, X=X.data_ptr(), truth=truth.data_ptr(), buf=buf.data_ptr(),
             cost=cost.data_ptr(), nlayers=None):
        w = (C.c_int64 * len(widths))(*widths)
        a = (C.c_int32 * len(acts))(*acts)
        return L.tns_hip_mlp_train_step(hip.ctx, len(acts) if nlayers is None else nlayers, w, a,
                                        0, B, X, truth, 1e-2, 0.9, 1e-4, buf, cost)

    ok = ([16, 8, 4], [1, 4])
    assert call(*ok, 1) == ERR_ARG                                  # batch 1
    assert call([16], [4], 4, nlayers=0) == ERR_ARG                 # no layer
    assert call([8] * 18, [1] * 16 + [4], 4) == ERR_ARG             # 17 layers
    assert call([16, 0, 4], [1, 4], 4) == ERR_ARG                   # a zero width
    assert call([16, 8, 0], [1, 4], 4) == ERR_ARG
    assert call([0, 8, 4], [1, 4], 4) == ERR_ARG
    assert call([8, 569, 10], [1, 4], 8) == ERR_ARG                 # 9*8*569 = 40968 > 40960
    assert call([16, 8, 4], [2, 4], 4) == ERR_UNSUPPORTED           # activation 2
    assert call(*ok, 4, X=None) == ERR_ARG
    assert call(*ok, 4, truth=None) == ERR_ARG
    assert call(*ok, 4, buf=None) == ERR_ARG
    assert call(*ok, 4, cost=None) == ERR_ARG
    hip.finish()
    assert bool((buf == float(SENT)).all()) and float(cost.item()) == float(SENT)
    # next to the refused [8, 569, 10] at batch 8: 9*3*1517 = 40959 is accepted
    w, a = [9, 1517], [4]
    assert L.tns_mlp_buffer_floats(1, (C.c_int64 * 2)(*w), 0, 3) <= n
    buf.zero_()
    assert call(w, a, 3) == 0
    hip.finish()
    assert np.isfinite(float(cost.item())) and float(cost.item()) != float(SENT)
