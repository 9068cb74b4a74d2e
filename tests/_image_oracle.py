"""NumPy float32 restatement of the reference's image preprocessing, the
expected values of tests/test_gpu_image.py and tests/test_gpu_image_net.py:

  resize         TImageData.resize (source/ntypes.pas:837-883), with its `part`
                 intermediate, pass for pass
  letterbox      TImageData.letterBox / letterBoxEx (899-947) with Embed
                 (885-897)
  byte_table     the loaders' byte -> single conversion: FPC's TFPColor word
                 over $ff00 (749-752), Delphi's byte over $ff (716-718)
  truth_rows     loadVOCBatch's box mapping (Samples/FPC/MSCOCO_Yolo/
                 MSCOCOYolo.pas:461-480)

Every array is float32 and every NumPy operation on float32 operands rounds
once, which is the reference's arithmetic: singles, no FMA.  integer / integer
in Pascal is a real (double) and is rounded when it is stored to a single.
"""
import numpy as np

F = np.float32
D = np.float64


def byte_table(kind="fpc"):
    b = np.arange(256)
    if not isinstance(kind, str):
        t = np.asarray(kind, dtype=F)
        assert t.shape == (256,)
        return t
    if kind == "fpc":       # img.Colors[..].Red / $ff00; an 8-bit sample b is the word b*257
        return (D(b * 257) / D(0xff00)).astype(F)
    if kind == "255":       # p.r / $ff
        return (D(b) / D(0xff)).astype(F)
    raise ValueError(kind)


def planar_from_bytes(img, channels, table="fpc"):
    """uint8 [h, w, pixel bytes] -> float32 [channels, h, w], channel k from
    byte k of a pixel."""
    return np.ascontiguousarray(byte_table(table)[img[:, :, :channels]].transpose(2, 0, 1))


def scale(n_src, n_dst):
    """w_scale := (self.w-1) / (aWidth-1), a real stored to a single (846-847)"""
    return F(D(n_src - 1) / D(n_dst - 1))


def resize(img, aW, aH):
    """TImageData.resize (837-883); img float32 [c, h, w] -> [c, aH, aW]."""
    img = np.asarray(img, dtype=F)
    c, h, w = img.shape
    assert aW >= 2 and aH >= 2
    w_scale, h_scale = scale(w, aW), scale(h, aH)
    part = np.empty((c, h, aW), F)
    if w == 1:                                       # 853-854
        part[:] = img[:, :, :1]
    else:
        sx = np.arange(aW - 1, dtype=F) * w_scale    # 857
        ix = np.trunc(sx).astype(np.int64)           # 858
        dx = sx - ix.astype(F)                       # 859
        assert sx.dtype == F and dx.dtype == F and ix.max() + 1 <= w - 1
        part[:, :, :aW - 1] = (F(1) - dx) * img[:, :, ix] + dx * img[:, :, ix + 1]   # 860
        part[:, :, aW - 1] = img[:, :, w - 1]        # 853-854
    sy = np.arange(aH, dtype=F) * h_scale            # 867
    iy = np.trunc(sy).astype(np.int64)               # 868
    dy = sy - iy.astype(F)                           # 869
    assert iy.max() <= h - 1
    res = (F(1) - dy)[None, :, None] * part[:, iy, :]          # 872-873
    if h > 1:                                        # 875-876: not the last row
        n = aH - 1
        assert iy[:n].max() + 1 <= h - 1
        res[:, :n, :] += dy[:n][None, :, None] * part[:, iy[:n] + 1, :]   # 879-880
    assert res.dtype == F
    return np.ascontiguousarray(res)    # (the row gather leaves a permuted layout)


def last_row(img, aH):
    """What resize leaves in its last row, from the formula alone:
    (1-dy) * P(iy) with sy = single(aH-1) * h_scale (no second term, 875);
    returns (row [c, w] for a same-width resize, iy, dy)."""
    c, h, w = img.shape
    sy = F(aH - 1) * scale(h, aH)
    iy = int(np.trunc(sy))
    dy = sy - F(iy)
    return (F(1) - dy) * np.asarray(img, F)[:, iy, :], iy, dy


def letterbox_geometry(w, h, aW, aH):
    """letterBoxEx's integers and ratio (922-947): (new_w, new_h, dx, dy, ratio)."""
    if D(aW) / D(w) < D(aH) / D(h):                  # 929
        new_w, new_h, ratio = aW, (h * aW) // w, F(D(aW) / D(w))
    else:
        new_h, new_w, ratio = aH, (w * aH) // h, F(D(aH) / D(h))
    return new_w, new_h, (aW - new_w) // 2, (aH - new_h) // 2, ratio


def letterbox(img, aW, aH):
    """letterBoxEx: (image [c, aH, aW], (new_w, new_h, dx, dy, ratio))."""
    c, h, w = img.shape
    new_w, new_h, dx, dy, ratio = letterbox_geometry(w, h, aW, aH)
    out = np.full((c, aH, aW), F(0.5))               # 943
    out[:, dy:dy + new_h, dx:dx + new_w] = resize(img, new_w, new_h)   # Embed, 885-897
    return out, (new_w, new_h, dx, dy, ratio)


def truth_rows(objects, dx, dy, ratio, net_w, net_h, max_boxes):
    """loadVOCBatch 461-480 for one image: objects (xmin, ymin, xmax, ymax,
    class) -> float32 [max_boxes, 6]."""
    out = np.zeros((max_boxes, 6), F)
    for j, (xmin, ymin, xmax, ymax, cls) in enumerate(objects):
        left = dx + int(np.trunc(F(xmin) * F(ratio)))      # 467
        top = dy + int(np.trunc(F(ymin) * F(ratio)))
        right = dx + int(np.trunc(F(xmax) * F(ratio)))
        bottom = dy + int(np.trunc(F(ymax) * F(ratio)))
        out[j, 0] = F(D(left + right) / D(2 * net_w))      # 472
        out[j, 1] = F(D(top + bottom) / D(2 * net_h))
        out[j, 2] = F(D(right - left) / D(net_w))
        out[j, 3] = F(D(bottom - top) / D(net_h))
        out[j, 4] = F(cls)                                 # 480
    return out
