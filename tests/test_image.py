"""The image oracle (tests/_image_oracle.py) held against what can be known
without the reference's binary: identities, an independent bilinear resize,
the bottom-row quirk from its formula, letterbox geometry and a truth mapping
worked by hand; the host function tensorium_amd.darknet.letterbox_truth
against the oracle's; and the new entry points' null-context guard."""
import numpy as np
import pytest

import _image_oracle as oracle

F = np.float32
D = np.float64


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _image(seed, c, h, w):
    return np.random.default_rng(seed).random((c, h, w), dtype=F)


@pytest.mark.parametrize("c,h,w", [(3, 37, 53), (1, 2, 9), (2, 9, 2), (4, 2, 2)])
def test_resize_to_own_size_is_identity(c, h, w):
    """w_scale = h_scale = 1: sx = x, dx = 0, (1-0)*a + 0*b = a, bit for bit."""
    img = _image(1, c, h, w)
    assert np.array_equal(_bits(oracle.resize(img, w, h)), _bits(img))


def _has_quirk(h, aH):
    sy = F(aH - 1) * oracle.scale(h, aH)
    return sy < F(h - 1)


@pytest.mark.parametrize("src,dst", [((53, 37), (32, 32)), ((53, 37), (19, 13)),
                                     ((53, 37), (101, 77)), ((9, 1), (6, 6)), ((1, 9), (6, 6))])
def test_agrees_with_align_corners_bilinear(src, dst):
    """An independent bilinear resize of the same float32 data: fewer than
    ten single roundings a side, each <= 2^-24 on data in [0, 1], so 2e-6
    absolute; 1.2e-7 at most on these cases.  (torch forms the source
    coordinate x * (w-1)/(aW-1) in single too.  Against a double
    interpolation the single coordinate's error of up to 52 * 2^-24 pixels
    times the slope between neighbours shows instead: 2e-6 .. 3e-6 on the
    53x37 cases, which is the reference's arithmetic and not the oracle's.)"""
    import torch
    (w, h), (aW, aH) = src, dst
    assert not _has_quirk(h, aH)
    img = _image(2, 3, h, w)
    want = torch.nn.functional.interpolate(torch.from_numpy(img)[None], size=(aH, aW),
                                           mode="bilinear", align_corners=True)[0].numpy()
    got = oracle.resize(img, aW, aH)
    err = np.abs(got.astype(D) - want).max()
    print("max |d|", err)
    assert err <= 2e-6


def test_sizes_named_for_the_bottom_row_quirk_have_it():
    for h, aH in ((2, 42), (16, 416), (479, 416), (481, 416), (46, 608)):
        assert _has_quirk(h, aH), (h, aH)
    for h, aH in ((37, 32), (37, 13), (37, 77), (53, 37)):
        assert not _has_quirk(h, aH), (h, aH)


def test_bottom_row_16_to_416_is_near_black():
    """single(415) * single(15/415) rounds below 15: the last row is
    (1-dy)*P(14) with dy just below 1, not P(15)."""
    img = _image(3, 3, 16, 21)
    res = oracle.resize(img, 21, 416)                 # same width: P(y) = the source row
    row, iy, dy = oracle.last_row(img, 416)
    assert iy == 14 and F(0.999) < dy < F(1)
    assert np.array_equal(_bits(res[:, -1, :]), _bits(row))
    assert res[:, -1, :].max() < 1e-5 and img[:, 15, :].min() > 1e-4
    # the row above is an ordinary blend of rows 14 and 15
    assert res[:, -2, :].min() > 1e-4


def test_byte_tables():
    fpc, d = oracle.byte_table("fpc"), oracle.byte_table("255")
    assert fpc.dtype == F and fpc[0] == 0 and d[0] == 0 and d[255] == 1
    assert fpc[255] == F(65535 / 65280) and fpc[255] > 1
    assert fpc[1] == F(257 / 65280) and d[128] == F(128 / 255)
    img = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    p = oracle.planar_from_bytes(img, 3, "255")
    assert p.shape == (3, 2, 3) and p[2, 1, 0] == d[img[1, 0, 2]]


def test_letterbox_geometry_by_hand():
    g = oracle.letterbox_geometry
    assert g(500, 375, 416, 416) == (416, 312, 0, 52, F(416 / 500))
    assert g(375, 500, 416, 416) == (312, 416, 52, 0, F(416 / 500))
    assert g(30, 30, 32, 32) == (32, 32, 0, 0, F(32 / 30))         # square: the else branch
    assert g(50, 20, 32, 32) == (32, 12, 0, 10, F(32 / 50))
    assert g(20, 50, 32, 32) == (12, 32, 10, 0, F(32 / 50))
    assert g(1000, 1, 32, 32)[1] == 0                               # new_h = 0: refused on the device
    for r in (g(500, 375, 416, 416)[4], g(30, 30, 32, 32)[4]):
        assert isinstance(r, F)
    assert g(500, 375, 416, 416)[4] == F(0.832)


def test_letterbox_border_and_content():
    img = _image(4, 3, 20, 50)
    out, (nw, nh, dx, dy, _) = oracle.letterbox(img, 32, 32)
    assert (nw, nh, dx, dy) == (32, 12, 0, 10)
    assert (out[:, :10] == F(0.5)).all() and (out[:, 22:] == F(0.5)).all()
    assert np.array_equal(_bits(out[:, 10:22]), _bits(oracle.resize(img, 32, 12)))


def test_truth_mapping_by_hand():
    """500x375 -> 416^2: ratio = single(0.832), dx = 0, dy = 52.  The box
    (48, 240, 195, 371) of class 11: 48*0.832 = 39.936 -> 39; 240*0.832 =
    199.68 -> 199 + 52 = 251; 195*0.832 = 162.24 -> 162; 371*0.832 = 308.672
    -> 308 + 52 = 360.  x = (39+162)/832, y = (251+360)/832, w = 123/416,
    h = 109/416."""
    _, _, dx, dy, ratio = oracle.letterbox_geometry(500, 375, 416, 416)
    rows = oracle.truth_rows([(48, 240, 195, 371, 11)], dx, dy, ratio, 416, 416, 3)
    want = np.zeros((3, 6), F)
    want[0] = (F(201 / 832), F(611 / 832), F(123 / 416), F(109 / 416), 11, 0)
    assert np.array_equal(_bits(rows), _bits(want))


def test_letterbox_truth_matches_the_oracle():
    from tensorium_amd import darknet as dn
    rng = np.random.default_rng(5)
    sizes = [(500, 375), (375, 500), (64, 64), (353, 500)]
    boxes, placed, want = [], [], []
    for n, (w, h) in enumerate(sizes):
        nw, nh, dx, dy, ratio = oracle.letterbox_geometry(w, h, 416, 416)
        placed.append(dn.Placement(nw, nh, dx, dy, w, h, ratio))
        objs = []
        for _ in range(n + 1):
            x0, x1 = sorted(rng.integers(0, w, 2).tolist())
            y0, y1 = sorted(rng.integers(0, h, 2).tolist())
            objs.append((x0, y0, x1, y1, int(rng.integers(0, 20))))
        boxes.append(objs)
        want.append(oracle.truth_rows(objs, dx, dy, ratio, 416, 416, 6))
    got = dn.letterbox_truth(boxes, placed, 416, 416, 6)
    assert got.dtype == F and got.shape == (4, 6, 6)
    assert np.array_equal(_bits(got), _bits(np.stack(want)))
    assert (got[0, 1:] == 0).all()                    # zero rows after the last
    skipped = dn.letterbox_truth([[None, boxes[0][0]]], placed[:1], 416, 416, 6)
    assert (skipped[0, 0] == 0).all() and np.array_equal(_bits(skipped[0, 1]), _bits(got[0, 0]))
    with pytest.raises(ValueError, match="max_boxes"):
        dn.letterbox_truth([boxes[3]], placed[3:], 416, 416, 3)


def test_null_ctx_rejected(hiplib):
    """As tests/test_abi.py::test_null_ctx_rejected: TNS_ERR_ARG, nothing touched."""
    assert hiplib.tns_image_bytes_to_input(None, 1, None, None, 3, 3, 0, None, 32, 32, 0, None,
                                           None) == 1
    assert hiplib.tns_image_floats_to_input(None, 1, None, None, 3, 32, 32, 0, None, None) == 1
    hiplib.tns_clear_error()
