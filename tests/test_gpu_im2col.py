"""im2col / col2im on the GPU vs the oracle (sim2Col ntensors.pas:11415-11532,
scol2im 11650-11879).  Bar: bit-exact (memcmp) for im2col; col2im is a
gather that adds in the reference's single-threaded order => bit-exact too."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GEOS = [  # C, H, W, k, pad, stride, dil
    (3, 7, 5, 3, 1, 1, 1), (5, 9, 11, 3, 1, 2, 1), (3, 8, 8, 1, 0, 1, 1), (2, 10, 7, 3, 0, 2, 2),
    (5, 13, 13, 3, 1, 1, 2), (3, 6, 9, 1, 0, 2, 1), (4, 16, 16, 3, 1, 2, 1), (1, 5, 5, 5, 2, 1, 1),
    (3, 416 // 8, 416 // 8, 3, 1, 1, 1), (2, 3, 3, 3, 0, 1, 1), (2, 4, 4, 3, 0, 3, 2),
]


@pytest.mark.parametrize("geo", GEOS)
@pytest.mark.parametrize("batch", [1, 3])
def test_im2col_bit_exact(hip, torch_cuda, ora, geo, batch):
    C, H, W, k, p, s, d = geo
    x = ora.uniform(batch * C * H * W, 3, sum(geo))
    ref = ora.im2col(C, H, W, k, k, p, p, s, s, d, d, x, batch=batch)
    if ref.size == 0:
        return
    dx = torch_cuda.from_numpy(x).cuda()
    dcol = torch_cuda.full(ref.shape, float("nan"), device="cuda")
    hip.im2colStridedBatched(C, H, W, k, k, p, p, s, s, d, d, dx, C * H * W, 0, dcol,
                             ref[0].size, 0, batch)
    hip.finish()
    assert dcol.cpu().numpy().tobytes() == ref.tobytes()


def test_im2col_single_with_offsets(hip, torch_cuda, ora):
    C, H, W, k, p, s, d = 3, 9, 9, 3, 1, 2, 1
    x = ora.uniform(7 + C * H * W, 3, 99)
    ref = ora.im2col(C, H, W, k, k, p, p, s, s, d, d, x[7:].copy())
    dx = torch_cuda.from_numpy(x).cuda()
    dcol = torch_cuda.zeros(5 + ref.size, device="cuda")
    hip.im2col(C, H, W, k, k, p, p, s, s, d, d, dx, 7, dcol, 5)
    hip.finish()
    assert dcol.cpu().numpy()[5:].tobytes() == ref.ravel().tobytes()


@pytest.mark.parametrize("geo", GEOS)
@pytest.mark.parametrize("batch", [1, 2])
def test_col2im_bit_exact(hip, torch_cuda, ora, geo, batch):
    C, H, W, k, p, s, d = geo
    oh = ora.out_dim(H, p, k, d, s)
    ow = ora.out_dim(W, p, k, d, s)
    if oh <= 0 or ow <= 0:
        return
    col = ora.uniform(batch * C * k * k * oh * ow, 4, sum(geo))
    base = ora.uniform(batch * C * H * W, 5, sum(geo))
    ref = ora.col2im(C, H, W, k, k, p, p, s, s, d, d, col.copy(), base.copy(), batch=batch)
    dcol = torch_cuda.from_numpy(col).cuda()
    dim = torch_cuda.from_numpy(base.copy()).cuda()
    hip.col2imStridedBatched(C, H, W, k, k, p, p, s, s, d, d, dcol, col.size // batch, 0, dim,
                             C * H * W, 0, batch)
    hip.finish()
    assert np.array_equal(dim.cpu().numpy(), ref)


# per-axis windows: kH != kW, padH != padW, sY != sX, dY != dX on H != W
# planes.  (4,12,9, 3,3, ..., 2,1, ...) is a 3x3 window with sY != sX: col2im
# takes col2im_fast_kernel<0> (runtime strides), not the k3 kernels;
# (2,8,15, 3,3, 2,0, 1,1, 1,2) takes col2im_k3_kernel<1> with dY != dX.
ANISO_GEOS = [  # C, H, W, kH, kW, padH, padW, sY, sX, dY, dX
    (3, 9, 14, 3, 2, 1, 0, 1, 2, 1, 1), (2, 11, 8, 1, 3, 0, 2, 2, 1, 1, 2),
    (2, 10, 13, 2, 3, 1, 1, 3, 1, 2, 1), (1, 7, 16, 3, 1, 0, 0, 1, 3, 2, 1),
    (4, 12, 9, 3, 3, 1, 1, 2, 1, 1, 1), (2, 8, 15, 3, 3, 2, 0, 1, 1, 1, 2),
]


def _out_dim(inp, pad, k, dil, stride):   # oracle.out_dim (Pascal div truncates toward zero)
    v = inp + 2 * pad - (dil * (k - 1) + 1)
    q = abs(v) // stride
    return (q if v >= 0 else -q) + 1


for _g in ANISO_GEOS:
    _C, _H, _W, _kH, _kW, _pH, _pW, _sY, _sX, _dY, _dX = _g
    _oh, _ow = _out_dim(_H, _pH, _kH, _dY, _sY), _out_dim(_W, _pW, _kW, _dX, _sX)
    assert _H != _W and _oh != _ow and _oh > 0 and _ow > 0, _g
    assert (_kH, _pH, _sY, _dY) != (_kW, _pW, _sX, _dX), _g


@pytest.mark.parametrize("geo", ANISO_GEOS)
@pytest.mark.parametrize("batch", [1, 3])
def test_im2col_per_axis_bit_exact(hip, torch_cuda, ora, geo, batch):
    C, H, W = geo[:3]
    x = ora.uniform(batch * C * H * W, 3, 100 + sum(geo))
    ref = ora.im2col(*geo, x, batch=batch)
    dx = torch_cuda.from_numpy(x).cuda()
    dcol = torch_cuda.full(ref.shape, float("nan"), device="cuda")
    hip.im2colStridedBatched(*geo, dx, C * H * W, 0, dcol, ref[0].size, 0, batch)
    hip.finish()
    assert dcol.cpu().numpy().tobytes() == ref.tobytes()


@pytest.mark.parametrize("geo", ANISO_GEOS)
@pytest.mark.parametrize("batch", [1, 2])
def test_col2im_per_axis_bit_exact(hip, torch_cuda, ora, geo, batch):
    C, H, W, kH, kW, pH, pW, sY, sX, dY, dX = geo
    oh, ow = ora.out_dim(H, pH, kH, dY, sY), ora.out_dim(W, pW, kW, dX, sX)
    col = ora.uniform(batch * C * kH * kW * oh * ow, 4, 100 + sum(geo))
    base = ora.uniform(batch * C * H * W, 5, 100 + sum(geo))
    ref = ora.col2im(*geo, col.copy(), base.copy(), batch=batch)
    dcol = torch_cuda.from_numpy(col).cuda()
    dim = torch_cuda.from_numpy(base.copy()).cuda()
    hip.col2imStridedBatched(*geo, dcol, col.size // batch, 0, dim, C * H * W, 0, batch)
    hip.finish()
    assert np.array_equal(dim.cpu().numpy(), ref)


# The plain im2col_kernel<VEC> of launch_im2col, taken when the row-staged
# form's R rows of Wp = W + 2*pad floats do not fit 64 KB of LDS:
#  (2,4,4200,3,1,1,1): oh x ow = 4 x 4200, ohw = 16800 (a multiple of 4: the
#    float4 form); R = max(1, 4096 / 4200) = 1 < oh, rounded up to 4 rows;
#    4 * 4202 * 4 = 67232 bytes > 65536  => im2col_kernel<4>
#  (1,3,16390,3,1,1,1): oh x ow = 3 x 16390, ohw = 49170 (not a multiple of 4:
#    the scalar form); R = max(1, 2048 / 16390) = 1 < oh; 1 * 16392 * 4 =
#    65568 bytes > 65536  => im2col_kernel<1>
WIDE_GEOS = [(2, 4, 4200, 3, 1, 1, 1), (1, 3, 16390, 3, 1, 1, 1)]

for _C, _H, _W, _k, _p, _s, _d in WIDE_GEOS:
    _oh, _ow = _out_dim(_H, _p, _k, _d, _s), _out_dim(_W, _p, _k, _d, _s)
    _vec = (_oh * _ow) % 4 == 0
    _R = max(1, (4096 if _vec else 2048) // _ow)
    assert _R < _oh
    if _vec:
        _R = max(4, _R & ~3)
    assert _R * (_W + 2 * _p) * 4 > 64 * 1024, (_C, _H, _W)
assert (4 * 4200) % 4 == 0 and (3 * 16390) % 4 != 0


@pytest.mark.parametrize("geo", WIDE_GEOS)
@pytest.mark.parametrize("batch", [1, 3])
def test_im2col_wide_rows_plain_kernel(hip, torch_cuda, ora, geo, batch):
    C, H, W, k, p, s, d = geo
    x = ora.uniform(batch * C * H * W, 3, 200 + C)
    ref = ora.im2col(C, H, W, k, k, p, p, s, s, d, d, x, batch=batch)
    dx = torch_cuda.from_numpy(x).cuda()
    dcol = torch_cuda.full(ref.shape, float("nan"), device="cuda")
    hip.im2colStridedBatched(C, H, W, k, k, p, p, s, s, d, d, dx, C * H * W, 0, dcol,
                             ref[0].size, 0, batch)
    hip.finish()
    assert dcol.cpu().numpy().tobytes() == ref.tobytes()


def test_host_api_im2col_col2im(hiplib, torch_cuda, ora):
    from tensorium_amd.ntensors import bind_hip_op_table
    ops = bind_hip_op_table()
    C, H, W, k, p, s, d, batch = 3, 11, 10, 3, 1, 2, 1, 2
    x = ora.uniform(batch * C * H * W, 6, 0)
    ref = ora.im2col(C, H, W, k, k, p, p, s, s, d, d, x, batch=batch)
    col = np.zeros_like(ref)
    ops.im2colStridedBatchedvv(C, H, W, k, k, p, p, s, s, d, d, x.ctypes.data, C * H * W, 0,
                               col.ctypes.data, ref[0].size, 0, batch)
    assert hiplib.tns_last_error() == b""
    assert col.tobytes() == ref.tobytes()
    base = ora.uniform(C * H * W, 7, 0)
    im = base.copy()
    ops.col2imvv(C, H, W, k, k, p, p, s, s, d, d, ref[0].ctypes.data, 0, im.ctypes.data, 0, 1, 0)
    want = ora.col2im(C, H, W, k, k, p, p, s, s, d, d, ref[0].copy(), base.copy())
    assert np.array_equal(im, want)


def test_im2col_yolo_first_layer_full_size(hip, torch_cuda, ora):
    # BASELINE size: 8 x 3 x 416 x 416, k3 s1 p1 (col 27 x 173056 per image)
    batch, C, H = 8, 3, 416
    x = ora.uniform(batch * C * H * H, 3, 0, 0.0, 1.0)
    ref = ora.im2col(C, H, H, 3, 3, 1, 1, 1, 1, 1, 1, x, batch=batch)
    dx = torch_cuda.from_numpy(x).cuda()
    dcol = torch_cuda.empty(ref.shape, device="cuda")
    hip.im2colStridedBatched(C, H, H, 3, 3, 1, 1, 1, 1, 1, 1, dx, C * H * H, 0, dcol,
                             ref[0].size, 0, batch)
    hip.finish()
    assert dcol.cpu().numpy().tobytes() == ref.tobytes()


def test_host_api_im2col_col2im_per_axis(hiplib, torch_cuda, ora):
    from tensorium_amd.ntensors import bind_hip_op_table
    ops = bind_hip_op_table()
    geo = (3, 9, 14, 3, 2, 1, 0, 1, 2, 1, 1)
    C, H, W = geo[:3]
    batch = 2
    x = ora.uniform(batch * C * H * W, 6, 1)
    ref = ora.im2col(*geo, x, batch=batch)
    col = np.zeros_like(ref)
    ops.im2colStridedBatchedvv(*geo, x.ctypes.data, C * H * W, 0, col.ctypes.data, ref[0].size, 0,
                               batch)
    assert hiplib.tns_last_error() == b""
    assert col.tobytes() == ref.tobytes()
    base = ora.uniform(C * H * W, 7, 1)
    im = base.copy()
    ops.col2imvv(*geo, ref[0].ctypes.data, 0, im.ctypes.data, 0, 1, 0)
    want = ora.col2im(*geo, ref[0].copy(), base.copy())
    assert np.array_equal(im, want)
