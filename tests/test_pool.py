"""Pooling without a GPU: the darknet plan with [maxpool] / [local_avgpool]
layers (parseMaxPool / parseLocalAvgPool, nparser.pas:248-292; shapes
nMaxPoolLayer.pas:107-109), the yolov3-tiny generator, the CPU checker
(tests/_pool_oracle.py) on hand-checked cases, and the Pascal binding's
text."""
import re
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from tensorium_amd import darknet as dn

import _pool_oracle as po

ROOT = Path(__file__).resolve().parents[1]
PAS = ROOT / "pascal" / "nnHip.pas"
FLT_MAX = np.float32(np.finfo(np.float32).max)


def _net(body, size=8, channels=4):
    return dn.Network(dn.parse_cfg(f"[net]\nbatch=1\nwidth={size}\nheight={size}\n"
                                   f"channels={channels}\n{body}"))


def test_yolov3_tiny_plan():
    net = dn.Network(dn.parse_cfg(dn.yolov3_tiny_cfg(416)))
    kinds = Counter(l.kind for l in net.layers)
    assert kinds == {"convolutional": 13, "maxpool": 6, "route": 2, "upsample": 1, "yolo": 2}
    pools = [l for l in net.layers if l.kind == "maxpool"]
    assert [(l.h, l.out_h) for l in pools] == [(416, 208), (208, 104), (104, 52), (52, 26),
                                               (26, 13), (13, 13)]
    last = pools[-1]   # size 2, stride 1, padding 1: 13x13 stays 13x13
    assert (last.size, last.stride_x, last.stride_y, last.pad) == (2, 1, 1, 1)
    assert (last.out_c, last.out_h, last.out_w) == (512, 13, 13)
    assert all((l.size, l.stride_x, l.stride_y, l.pad) == (2, 2, 2, 1) for l in pools[:-1])
    yolos = [l for l in net.layers if l.kind == "yolo"]
    assert [(l.h, l.w) for l in yolos] == [(13, 13), (26, 26)]
    assert all(l.c == 255 and l.anchors == 3 and l.classes == 80 for l in yolos)
    # the second scale concatenates the upsampled 128 channels with layer 8's 256
    route = [l for l in net.layers if l.kind == "route"][1]
    assert route.inputs == (19, 8) and (route.out_c, route.out_h) == (384, 26)


def test_yolov3_tiny_plan_other_sizes():
    net = dn.Network(dn.parse_cfg(dn.yolov3_tiny_cfg(64, batch=2, classes=2)))
    assert net.batch == 2
    yolos = [l for l in net.layers if l.kind == "yolo"]
    assert [(l.c, l.h) for l in yolos] == [(21, 2), (21, 4)]


@pytest.mark.parametrize("kind", ["maxpool", "max", "local_avgpool"])
def test_pool_option_defaults(kind):
    # nothing given: stride 1, size = stride, padding = size - 1
    l = _net(f"[{kind}]\n").layers[0]
    assert l.kind == ("local_avgpool" if kind == "local_avgpool" else "maxpool")
    assert (l.size, l.stride_x, l.stride_y, l.pad, l.out_h, l.out_w) == (1, 1, 1, 0, 8, 8)
    # size defaults to stride, padding to size - 1
    l = _net(f"[{kind}]\nstride=2\n").layers[0]
    assert (l.size, l.stride_x, l.stride_y, l.pad, l.out_h, l.out_w) == (2, 2, 2, 1, 4, 4)
    # stride_x / stride_y default to stride, each on its own
    l = _net(f"[{kind}]\nsize=3\nstride=2\nstride_y=1\n").layers[0]
    assert (l.size, l.stride_x, l.stride_y, l.pad) == (3, 2, 1, 2)
    assert (l.out_c, l.out_h, l.out_w) == (4, (8 + 2 - 3) // 1 + 1, (8 + 2 - 3) // 2 + 1)
    # explicit padding; a zero stride means the kernel size (nMaxPoolLayer.pas:79-82)
    l = _net(f"[{kind}]\nsize=3\nstride=2\npadding=0\nstride_x=0\n").layers[0]
    assert (l.stride_x, l.stride_y, l.pad, l.out_h, l.out_w) == (3, 2, 0, 3, 2)
    # a conv keeps both strides equal to its stride
    c = _net("[convolutional]\nfilters=2\nsize=3\nstride=2\npad=1\nactivation=leaky\n").layers[0]
    assert (c.stride, c.stride_x, c.stride_y) == (2, 2, 2)


@pytest.mark.parametrize("opt", ["maxpool_depth=1", "antialiasing=1", "antialiasing=2"])
def test_maxpool_depth_and_antialiasing_refused(opt):
    with pytest.raises(ValueError, match="maxpool_depth / antialiasing"):
        _net(f"[maxpool]\nsize=2\nstride=2\n{opt}\n")
    _net("[maxpool]\nsize=2\nstride=2\nmaxpool_depth=0\nantialiasing=0\n")


def test_oracle_hand_checked_3x3():
    """1x1x3x3, size 2, stride 1, padding 1: off = 0, out 3x3; the last row
    and column of windows reach past the input."""
    x = np.array([[1, 5, 2], [7, 3, 9], [4, 8, 6]], np.float32).reshape(1, 1, 3, 3)
    out, idx = po.maxpool_forward(x, 2, 1, 1, 1)
    assert out.reshape(3, 3).tolist() == [[7, 9, 9], [8, 9, 9], [8, 8, 6]]
    assert idx.reshape(3, 3).tolist() == [[3, 5, 5], [7, 5, 5], [7, 7, 8]]
    lo, li = po.maxpool_forward_loop(x, 2, 1, 1, 1)
    assert np.array_equal(lo, out) and np.array_equal(li, idx)
    avg = po.avgpool_forward(x, 2, 1, 1, 1)
    assert avg.reshape(3, 3).tolist() == [[4, 4.75, 5.5], [5.5, 6.5, 7.5], [6, 7, 6]]
    # backward from a non-zero state.delta: element 5 (the 9) is named by four
    # outputs, 7 (the 8) by three
    d = np.arange(1, 10, dtype=np.float32)
    sd = np.full(9, 100, np.float32)
    po.maxpool_backward(sd, idx, d)
    assert sd.tolist() == [100, 100, 100, 101, 100, 100 + 2 + 3 + 5 + 6, 100, 100 + 4 + 7 + 8,
                           109]
    sa = np.zeros(9, np.float32)
    po.avgpool_backward(sa, d, (1, 1, 3, 3), 2, 1, 1, 1)
    # input (1, 1) lies in windows 0, 1, 3, 4; the corner (2, 2) in 4, 5, 7, 8
    assert sa[4] == (1 + 2 + 4 + 5) / 4 and sa[8] == (5 + 6 + 8 + 9) / 4 and sa[0] == 0.25


def test_oracle_tie_first_in_scan_order_wins():
    x = np.array([[2, 2], [2, 2]], np.float32).reshape(1, 1, 2, 2)
    out, idx = po.maxpool_forward(x, 2, 2, 2, 0)
    assert out.ravel().tolist() == [2] and idx.ravel().tolist() == [0]
    x = np.array([[1, 3], [3, 3]], np.float32).reshape(1, 1, 2, 2)
    _, idx = po.maxpool_forward(x, 2, 2, 2, 0)
    assert idx.ravel().tolist() == [1]   # row 0's 3 before row 1's


def test_oracle_specials():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    x = np.array([[nan, nan, -inf, 1], [nan, nan, -FLT_MAX, nan]], np.float32).reshape(1, 1, 2, 4)
    out, idx = po.maxpool_forward(x, 2, 2, 2, 0)
    # all NaN: nothing is ever greater than -FLT_MAX
    assert out.ravel()[0] == -FLT_MAX and idx.ravel()[0] == -1
    assert out.ravel()[1] == 1 and idx.ravel()[1] == 3
    lo, li = po.maxpool_forward_loop(x, 2, 2, 2, 0)
    assert np.array_equal(lo, out) and np.array_equal(li, idx)
    # -inf and -FLT_MAX alone are not taken either
    y = np.array([[-inf, -FLT_MAX]], np.float32).reshape(1, 1, 1, 2)
    out, idx = po.maxpool_forward(y, 2, 2, 2, 1)
    assert out.ravel().tolist() == [-FLT_MAX] and idx.ravel().tolist() == [-1]
    z = np.array([[-inf, inf]], np.float32).reshape(1, 1, 1, 2)
    out, idx = po.maxpool_forward(z, 2, 2, 2, 1)
    assert out.ravel().tolist() == [inf] and idx.ravel().tolist() == [1]
    # the backward ignores -1
    sd = np.array([1, 2], np.float32)
    po.maxpool_backward(sd, np.array([-1, 1]), np.array([5, 7], np.float32))
    assert sd.tolist() == [1, 9]


def test_oracle_backward_add_at_is_the_plain_loop():
    """size 3, stride 1 (every input named by up to nine outputs), deltas of
    mixed magnitude: np.add.at adds element by element in ascending output
    index in float32, exactly as the loop; the reversed order differs."""
    rng = np.random.default_rng(7)
    x = (rng.integers(0, 4, (2, 3, 6, 7)) / 4).astype(np.float32)
    out, idx = po.maxpool_forward(x, 3, 1, 1, 2)
    lo, li = po.maxpool_forward_loop(x, 3, 1, 1, 2)
    assert np.array_equal(lo, out) and np.array_equal(li, idx)
    d = (rng.uniform(-1, 1, out.shape) * 10.0 ** rng.integers(-3, 4, out.shape)).astype(np.float32)
    sd0 = rng.uniform(-1, 1, x.shape).astype(np.float32)
    a, b, c = sd0.copy(), sd0.copy(), sd0.copy()
    po.maxpool_backward(a, idx, d)
    po.maxpool_backward_loop(b, idx, d)
    po.maxpool_backward(c, idx, d, descending=True)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)
    a, b, c = sd0.copy(), sd0.copy(), sd0.copy()
    po.avgpool_backward(a, d, x.shape, 3, 1, 1, 2)
    po.avgpool_backward_loop(b, d, x.shape, 3, 1, 1, 2)
    po.avgpool_backward(c, d, x.shape, 3, 1, 1, 2, descending=True)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)


def _method_body(src, name):
    i = src.index(f"procedure TNNHip<T>.{name}(")
    return src[src.index("begin", i):src.index("\nend;", i)]


def test_pascal_maxpool_methods_call_the_backend():
    src = PAS.read_text()
    fwd, bwd = _method_body(src, "forwardMaxPool"), _method_body(src, "backwardMaxPool")
    assert "raise" not in fwd
    assert "tns_hip_maxpool_forward(FCtx" in fwd
    # the bare TNNCuda-shaped call (no geometry) is refused, with the reason
    assert re.search(r"if kernelSize = 0 then\s+raise ENotSupportedException\.Create\("
                     r"'[^']*needs the layer geometry", bwd)
    assert bwd.count("raise") == 1
    assert "tns_hip_maxpool_backward(FCtx" in bwd
    for body in (fwd, bwd):
        assert "not on the hot path" not in body
    assert "tns_hip_avgpool_forward(FCtx" in _method_body(src, "forwardAvgPool")
    assert "tns_hip_avgpool_backward(FCtx" in _method_body(src, "backwardAvgPool")
    # TNNCuda's seven leading parameters, then the geometry with defaults
    assert re.search(r"procedure backwardMaxPool\(const aBatch, outC, outH, outW: SizeInt; "
                     r"output: TCUMem; const indexes, delta: TCUMem; const h: SizeInt = 0;", src)
    assert "const kernelSize: SizeInt = 0);" in src


@pytest.mark.parametrize("name", ["tns_hip_maxpool_forward", "tns_hip_maxpool_backward",
                                  "tns_hip_avgpool_forward", "tns_hip_avgpool_backward"])
def test_pascal_pool_externals(name):
    src = PAS.read_text()
    assert re.search(rf"function {name}\(ctx: PTnsCtx;[^)]*\): longint;\s*cdecl; external libtns;",
                     src)
    from tensorium_amd import _abi
    assert name in _abi.PROTOTYPES and name in _abi.header_symbols()
