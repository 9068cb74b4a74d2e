"""CPU restatement of TMaxPoolLayer's four loops (test infrastructure), the
checker for the HIP pooling kernels:

* ``maxpool_forward``  nMaxPoolLayer.pas:415-451: per output the window is
  scanned rows outer, columns inner, from max = -MaxSingle, max_i = -1, with a
  strict ``val > max``; out-of-range taps read as -MaxSingle; the stored index
  is the element index into the whole batch buffer (int64);
* ``avgpool_forward``  465-499: in-range taps summed in scan order in float32,
  then divided by their count;
* ``maxpool_backward`` 501-513: ``state.delta[indexes[i]] += delta[i]`` for i
  ascending, one float32 add at a time.  An index of -1 is skipped (the
  reference would write out of bounds; the backend ignores it, tns.h);
* ``avgpool_backward`` 515-542: outputs ascending, taps in scan order,
  ``state.delta[index] += delta[out] / (kernelSize*kernelSize)``.

The forwards walk the taps in scan order and are vectorised over the outputs;
the backwards use ``np.add.at`` (unbuffered, element by element in array
order, in the array's float32), with ``*_loop`` twins that are the plain
loops.  ``train_pass`` is tests/_darknet_oracle.py's walker plus the two pool
kinds.
"""
from __future__ import annotations

import numpy as np

from _darknet_oracle import upsample_backward

FLT_MAX = np.float32(np.finfo(np.float32).max)


def out_shape(h, w, size, sx, sy, padding):
    """nMaxPoolLayer.pas:107-109."""
    return (h + padding - size) // sy + 1, (w + padding - size) // sx + 1


def _taps(h, w, size, sx, sy, padding):
    """Per tap (n, m) in scan order: rows [outH], columns [outW] and the
    in-range mask [outH, outW]."""
    oh, ow = out_shape(h, w, size, sx, sy, padding)
    off = -(padding // 2)
    for n in range(size):
        for m in range(size):
            ch = off + np.arange(oh) * sy + n
            cw = off + np.arange(ow) * sx + m
            ok = ((ch >= 0) & (ch < h))[:, None] & ((cw >= 0) & (cw < w))[None, :]
            yield ch, cw, ok


def maxpool_forward(x: np.ndarray, size, sx, sy, padding):
    """x [B, C, H, W] float32 -> (out [B, C, outH, outW] float32, indexes int64)."""
    B, C, H, W = x.shape
    oh, ow = out_shape(H, W, size, sx, sy, padding)
    mx = np.full((B, C, oh, ow), -FLT_MAX, np.float32)
    mi = np.full((B, C, oh, ow), -1, np.int64)
    plane = (np.arange(B * C, dtype=np.int64) * (H * W)).reshape(B, C, 1, 1)
    with np.errstate(invalid="ignore"):
        for ch, cw, ok in _taps(H, W, size, sx, sy, padding):
            val = x[:, :, np.clip(ch, 0, H - 1)[:, None], np.clip(cw, 0, W - 1)[None, :]]
            val = np.where(ok, val, -FLT_MAX)
            index = plane + (ch[:, None].astype(np.int64) * W + cw[None, :])
            take = val > mx
            mx = np.where(take, val, mx)
            mi = np.where(take, index, mi)
    return mx, mi


def maxpool_forward_loop(x: np.ndarray, size, sx, sy, padding):
    """The plain loop (small shapes)."""
    B, C, H, W = x.shape
    oh, ow = out_shape(H, W, size, sx, sy, padding)
    off = -(padding // 2)
    flat = x.ravel()
    out = np.empty((B, C, oh, ow), np.float32)
    idx = np.empty((B, C, oh, ow), np.int64)
    for b in range(B):
        for k in range(C):
            for i in range(oh):
                for j in range(ow):
                    mx, mi = -FLT_MAX, -1
                    for n in range(size):
                        for m in range(size):
                            ch, cw = off + i * sy + n, off + j * sx + m
                            index = cw + W * (ch + H * (k + b * C))
                            val = flat[index] if 0 <= ch < H and 0 <= cw < W else -FLT_MAX
                            if val > mx:
                                mx, mi = val, index
                    out[b, k, i, j], idx[b, k, i, j] = mx, mi
    return out, idx


def avgpool_forward(x: np.ndarray, size, sx, sy, padding):
    B, C, H, W = x.shape
    oh, ow = out_shape(H, W, size, sx, sy, padding)
    avg = np.zeros((B, C, oh, ow), np.float32)
    cnt = np.zeros((oh, ow), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for ch, cw, ok in _taps(H, W, size, sx, sy, padding):
            val = x[:, :, np.clip(ch, 0, H - 1)[:, None], np.clip(cw, 0, W - 1)[None, :]]
            avg = np.where(ok, (avg + val).astype(np.float32), avg)
            cnt += ok
        return (avg / cnt.astype(np.float32)).astype(np.float32)


def maxpool_backward(sd: np.ndarray, idx: np.ndarray, delta: np.ndarray,
                     descending: bool = False) -> None:
    """sd (state.delta, any shape, float32, contiguous) accumulates in place.
    descending: the wrong order, for the tests' own sensitivity check."""
    assert sd.dtype == np.float32 and sd.flags.c_contiguous
    i, d = idx.ravel(), delta.ravel().astype(np.float32)
    keep = i >= 0
    i, d = i[keep], d[keep]
    if descending:
        i, d = i[::-1], d[::-1]
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(sd.reshape(-1), i, d)


def maxpool_backward_loop(sd: np.ndarray, idx: np.ndarray, delta: np.ndarray) -> None:
    s, ix, d = sd.reshape(-1), idx.ravel(), delta.ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        for o in range(ix.size):
            if ix[o] >= 0:
                s[ix[o]] = np.float32(s[ix[o]] + d[o])


def _avg_terms(shape_in, delta, size, sx, sy, padding):
    """(index, term) pairs of backwardAvgPool in the loop's order: output
    major, tap (scan order) minor."""
    B, C, H, W = shape_in
    oh, ow = out_shape(H, W, size, sx, sy, padding)
    term = (delta.reshape(B, C, oh, ow) / np.float32(size * size)).astype(np.float32)
    plane = (np.arange(B * C, dtype=np.int64) * (H * W)).reshape(B, C, 1, 1)
    ids, oks = [], []
    for ch, cw, ok in _taps(H, W, size, sx, sy, padding):
        ids.append(np.broadcast_to(plane + (ch[:, None].astype(np.int64) * W + cw[None, :]),
                                   term.shape))
        oks.append(np.broadcast_to(ok, term.shape))
    ids, oks = np.stack(ids, -1), np.stack(oks, -1)       # [B, C, oh, ow, taps]
    terms = np.broadcast_to(term[..., None], ids.shape)
    return ids[oks], terms[oks]                            # C order: output major


def avgpool_backward(sd: np.ndarray, delta: np.ndarray, shape_in, size, sx, sy, padding,
                     descending: bool = False) -> None:
    assert sd.dtype == np.float32 and sd.flags.c_contiguous
    i, t = _avg_terms(shape_in, delta, size, sx, sy, padding)
    if descending:
        i, t = i[::-1], t[::-1]
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(sd.reshape(-1), i, t)


def avgpool_backward_loop(sd: np.ndarray, delta: np.ndarray, shape_in, size, sx, sy,
                          padding) -> None:
    B, C, H, W = shape_in
    oh, ow = out_shape(H, W, size, sx, sy, padding)
    off = -(padding // 2)
    s, d = sd.reshape(-1), delta.ravel()
    kk = np.float32(size * size)
    for b in range(B):
        for k in range(C):
            for i in range(oh):
                for j in range(ow):
                    o = j + ow * (i + oh * (k + C * b))
                    for n in range(size):
                        for m in range(size):
                            ch, cw = off + i * sy + n, off + j * sx + m
                            if 0 <= ch < H and 0 <= cw < W:
                                index = cw + W * (ch + H * (k + b * C))
                                s[index] = np.float32(s[index] + np.float32(d[o] / kk))


def infer_pass(ora, net, params, x: np.ndarray):
    """oracle.darknet_forward (inference, BN folded into the convolutions)
    with the two pool kinds: every layer's output, flat."""
    B = net.batch
    outs = []
    prev = np.ascontiguousarray(x, np.float32).ravel()
    convs = iter(params)
    for l in net.layers:
        if l.kind == "convolutional":
            p = next(convs)
            w = np.ascontiguousarray(p.weights, np.float32).ravel().copy()
            b = np.ascontiguousarray(p.biases, np.float32).copy()
            if l.bn:
                sc, rm, rv = (np.ascontiguousarray(t, np.float32) for t in
                              (p.scales, p.rolling_mean, p.rolling_var))
                ora.lib().ora_fuse_batchnorm(l.filters, l.c * l.size * l.size, ora._p(w),
                                             ora._p(b), ora._p(sc), ora._p(rm), ora._p(rv))
            y = ora.conv_forward(prev.reshape(B, l.c, l.h, l.w), w, b, l.filters, l.size,
                                 l.stride, l.pad, l.activation).ravel()
        elif l.kind == "shortcut":
            y = ora.shortcut(prev, outs[l.inputs[0]], l.activation)
        elif l.kind == "route":
            y = ora.concat([outs[s] for s in l.inputs])
        elif l.kind == "upsample":
            y = ora.upsample(prev, B * l.c, l.h, l.w, l.stride, 1.0)
        elif l.kind == "yolo":
            y = ora.yolo_forward(prev, B, l.anchors, l.classes, l.h * l.w)
        elif l.kind == "maxpool":
            y = maxpool_forward(prev.reshape(B, l.c, l.h, l.w), l.size, l.stride_x, l.stride_y,
                                l.pad)[0].ravel()
        elif l.kind == "local_avgpool":
            y = avgpool_forward(prev.reshape(B, l.c, l.h, l.w), l.size, l.stride_x, l.stride_y,
                                l.pad).ravel()
        else:
            raise ValueError(l.kind)
        outs.append(np.ascontiguousarray(y, np.float32))
        prev = outs[-1]
    return outs


def train_pass(ora, net, params, x: np.ndarray, yolo_deltas, loss_scale: float = 1.0,
               quirk: int = 0, seed_delta=None):
    """tests/_darknet_oracle.py's train_pass with maxpool / local_avgpool
    layers: returns (outs, deltas, conv_state, indexes); indexes maps a
    maxpool's layer index to its stored indexes."""
    B = net.batch
    outs, state, indexes = [], {}, {}
    prev = x
    for l in net.layers:
        p4 = prev.reshape(B, l.c, l.h, l.w)
        if l.kind == "convolutional":
            p = params[len(state)]
            st = {"w": p.weights.copy(), "wu": np.zeros(p.weights.size, np.float32),
                  "bu": np.zeros(l.filters, np.float32)}
            if l.bn:
                rm, rv = p.rolling_mean.copy(), p.rolling_var.copy()
                out, m, v, xs, xn = ora.conv_forward_train(
                    p4, p.weights.ravel(), l.filters, l.size, l.stride, l.pad, l.activation,
                    p.scales, p.biases, rm, rv, 0.1, True, quirk=quirk)
                st.update(scales=p.scales, mean=m, var=v, x=xs.ravel(), xn=xn.ravel(), rm=rm,
                          rv=rv, su=np.zeros(l.filters, np.float32))
            else:
                out = ora.conv_forward(p4, p.weights.ravel(), p.biases, l.filters, l.size,
                                       l.stride, l.pad, l.activation)
            state[l.index] = st
            out = out.ravel()
        elif l.kind == "shortcut":
            out = ora.shortcut(prev.ravel(), outs[l.inputs[0]].ravel(), l.activation)
        elif l.kind == "route":
            out = ora.concat([outs[s] for s in l.inputs])
        elif l.kind == "upsample":
            out = ora.upsample(prev.ravel(), B * l.c, l.h, l.w, l.stride)
        elif l.kind == "yolo":
            out = ora.yolo_forward(prev.ravel(), B, l.anchors, l.classes, l.h * l.w)
        elif l.kind == "maxpool":
            out, indexes[l.index] = maxpool_forward(p4, l.size, l.stride_x, l.stride_y, l.pad)
        elif l.kind == "local_avgpool":
            out = avgpool_forward(p4, l.size, l.stride_x, l.stride_y, l.pad)
        else:
            raise ValueError(l.kind)
        outs.append(np.ascontiguousarray(out, dtype=np.float32).ravel())
        prev = outs[-1]
    deltas = [np.zeros(B * l.out_size, np.float32) for l in net.layers]
    ys = [l for l in net.layers if l.kind == "yolo"]
    for l, d in zip(ys, yolo_deltas):
        deltas[l.index][:] = np.asarray(d, np.float32).ravel()
    for i, d in (seed_delta or {}).items():
        deltas[i][:] = np.asarray(d, np.float32).ravel()
    for l in reversed(net.layers):
        i = l.index
        inp = (x if i == 0 else outs[i - 1]).reshape(B, l.c, l.h, l.w)
        sd = None if i == 0 else deltas[i - 1]
        d = deltas[i]
        if l.kind == "convolutional":
            st = state[i]
            if l.bn:
                md, vd = ora.conv_backward_bn(inp, st["w"].ravel(), l.filters, l.size, l.stride,
                                              l.pad, l.activation, outs[i], d, st["scales"],
                                              st["x"], st["xn"], st["mean"], st["var"], st["su"],
                                              st["wu"], sd, quirk=quirk)
                st.update(md=md, vd=vd)
            else:
                ora.conv_backward(inp, st["w"].ravel(), l.filters, l.size, l.stride, l.pad,
                                  l.activation, outs[i], d, st["bu"], st["wu"], sd)
        elif l.kind == "shortcut":
            ora.gradient(outs[i], l.activation, d)
            sd[:] = d + sd
            src = deltas[l.inputs[0]]
            src[:] = src + d
        elif l.kind == "route":
            off = 0
            for s in l.inputs:
                pt = deltas[s]
                pt[:] = pt + d[off:off + pt.size]
                off += pt.size
        elif l.kind == "upsample":
            upsample_backward(sd, d, B * l.c, l.h, l.w, l.stride)
        elif l.kind == "yolo":
            sd[:] = sd + (np.float32(loss_scale) * d).astype(np.float32)
        elif l.kind == "maxpool" and sd is not None:
            maxpool_backward(sd, indexes[i], d)
        elif l.kind == "local_avgpool" and sd is not None:
            avgpool_backward(sd, d, (B, l.c, l.h, l.w), l.size, l.stride_x, l.stride_y, l.pad)
    return outs, deltas, state, indexes
