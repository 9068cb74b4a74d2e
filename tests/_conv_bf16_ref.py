"""What the bf16 convolution tests share: test data, the float64 references of
the forward and of the backward's two products, and the derived error bounds.

The references convolve the bf16-rounded operands in float64.  A product of
two bf16 values is exact in fp32, so a kernel's only error is its fp32
accumulation, in whatever order, of n products and one more term (the bias or
the buffer's prior value): with S the same sum over absolute values and unit
roundoff U = 2^-23 (which covers a truncating accumulator),

    |got - ref| <= (n + 2) * U * S + U.

`draw_edges` gives data on which the rounding of the operands itself is under
test: exact ties, values a bf16 holds exactly, mantissas that carry into the
exponent and both zeros.  Subnormals, Inf, NaN and values that round to Inf
are left out on purpose: what the MFMA does with bf16 subnormals has not been
measured on this project, and the references here say nothing about it.
Everything drawn is finite, zero or of magnitude in [2^-20, 2].

The rounding and the tap order of the references can be replaced
(`rnd_*`, `swap`): tests/test_conv_bf16_ref.py uses that to show that the
bound tells a wrong rounding mode or a transposed kernel from the right one.
"""
import numpy as np

from tensorium_amd._abi import ACT

F = np.float32
U = 2.0 ** -23


def bf16_round(a):
    """float32 -> nearest-even bf16, as float32 (the upper 16 bits)."""
    u = np.ascontiguousarray(a, F).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(F)


def bf16_truncate(a):
    """The wrong rounding 1: the low 16 bits dropped."""
    u = np.ascontiguousarray(a, F).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(F)


def bf16_half_away(a):
    """The wrong rounding 2: nearest, ties up in magnitude (away from zero)."""
    u = np.ascontiguousarray(a, F).view(np.uint32).astype(np.uint64)
    u = ((u + 0x8000) >> 16) << 16
    return u.astype(np.uint32).view(F)


def draw(rng, *shape):
    v = rng.uniform(-1.0, 1.0, shape).astype(F)
    v[np.abs(v) < 2.0 ** -20] = 0.0
    return v


def draw_edges(rng, *shape):
    """fp32 data for the operand rounding: a quarter exact ties (low half
    0x8000, either parity of bit 16, either sign, magnitude in [1/4, 2)), a
    quarter values a bf16 holds exactly, 3% whose low half is 0xFFFF (the
    rounding carries through the mantissa, for 0x3F7FFFFF-like ones into the
    exponent), 3% each of +0.0 and -0.0, the rest uniform in (-1, 1)."""
    n = int(np.prod(shape, dtype=np.int64))
    u = draw(rng, n).view(np.uint32).copy()
    kind = rng.permutation(n) / n  # exact shares, whatever n
    # sign, an exponent of [1/4, 2), seven mantissa bits
    bits = lambda lo, up: rng.integers(lo, up, n, dtype=np.uint32)  # noqa: E731
    hi = (bits(0, 2) << 31) | (bits(125, 128) << 23) | (bits(0, 128) << 16)
    tie, exact, carry = kind < 0.25, (kind >= 0.25) & (kind < 0.5), (kind >= 0.5) & (kind < 0.53)
    u[tie] = hi[tie] | 0x8000
    u[exact] &= 0xFFFF0000
    # every fourth carry is 0x3F7FFFFF itself (or its negative): -> 1.0
    full = carry & (rng.integers(0, 4, n) == 0)
    u[carry] = hi[carry] | 0xFFFF
    u[full] = (hi[full] & 0x80000000) | 0x3F7FFFFF
    u[(kind >= 0.53) & (kind < 0.56)] = 0x00000000
    u[(kind >= 0.56) & (kind < 0.59)] = 0x80000000
    v = u.view(F).reshape(shape)
    a = np.abs(v)
    assert np.isfinite(v).all() and ((a == 0) | ((a >= 2.0 ** -20) & (a <= 2.0))).all()
    return v


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


# C, H, W, filters, k, stride, pad, batch: the shapes that run on draw_edges data
TIE_CASES = [
    (8, 6, 6, 8, 3, 1, 0, 1),       # below one tile, R = 16, K = 72
    (3, 10, 7, 16, 3, 1, 1, 2),     # K = 27, H != W
    (40, 9, 11, 18, 3, 2, 1, 2),    # stride 2, K = 360: the longest sums, the hardest to tell
    (32, 13, 13, 255, 1, 1, 0, 3),  # 1x1, 255 filters
]


def operands(case, edges=False):
    """A case's seeded operands and prior buffers, as a dict: x [B, C, H, W],
    w [filters, C*k*k], b [filters], d [B, filters, oh, ow], and wu0, sd0, bu0
    (weight_updates, state_delta and bias_updates before the call)."""
    C, H, W, filters, k, stride, pad, batch = case
    oh, ow = out_hw(H, W, k, stride, pad)
    rng = np.random.default_rng([filters, C, H, k, stride, pad, batch, int(edges)])
    new = draw_edges if edges else draw
    return dict(x=new(rng, batch, C, H, W), w=new(rng, filters, C * k * k), b=new(rng, filters),
                d=new(rng, batch, filters, oh, ow), wu0=new(rng, filters, C * k * k),
                sd0=new(rng, batch * C * H * W), bu0=new(rng, filters))


def _conv(torch, a, c, dtype=np.float64, **kw):
    return torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(a, dtype)),
                                      torch.from_numpy(np.ascontiguousarray(c, dtype)),
                                      **kw).numpy()


def activate(y, S, act):
    """The activation (tns_act.hpp's definitions) of the float64 y, and S scaled
    by the activation's largest slope."""
    if act == ACT["LOGISTIC"]:  # 1 / (1 + exp(-y)): slope <= 1/4
        return 1.0 / (1.0 + np.exp(-y)), S / 4
    if act in (ACT["LEAKY"], ACT["REVLEAKY"]):  # both: 0 > y ? 0.1f * y : y, slope <= 1
        return np.where(y < 0, 0.1 * y, y), S
    if act == ACT["RELU"]:
        return np.maximum(y, 0.0), S
    if act == ACT["HARDTAN"]:  # the clamp to [-1, 1]: slope <= 1, no rounding of its own
        return np.clip(y, -1.0, 1.0), S
    if act == ACT["TANH"]:
        # t = (px - nx) / (px + nx), px = fl(exp(y)), nx = fl(exp(-y)): slope <= 1, and the
        # five fp32 roundings of the formula cost at most (1/2 + 2|t|) U <= 2 U S + U, the
        # slack of the bound's "+ 2" and "+ U" (S >= |y| >= |t|; for |t| <= 1/4 the U alone)
        return np.tanh(y), S
    assert act == ACT["LINEAR"]
    return y, S


def reference_forward(torch, x, w, b, k, stride, pad, act, rnd_x=bf16_round, rnd_w=bf16_round,
                      swap=False, dtype=np.float64):
    """(ref, bound) of the layer in float64 from the rounded operands: x
    [B, C, H, W], w [filters, C*k*k], b [filters].  The bound is (K + 2) U S' + U
    with S = conv(|w~|, |x~|) + |b| and S' = S times the activation's largest
    slope (S / 4 for the logistic, S for the others: `activate`).  swap: the
    taps' ky and kx exchanged, a mistake to be told from the right order.
    dtype: float32 evaluates the same sums in fp32 instead."""
    w4 = w.reshape(w.shape[0], x.shape[1], k, k)
    xr, wr, b8 = rnd_x(x), rnd_w(w4), b.astype(dtype)[None, :, None, None]
    if swap:
        wr = wr.transpose(0, 1, 3, 2)
    y = _conv(torch, xr, wr, dtype, stride=stride, padding=pad) + b8
    S = _conv(torch, np.abs(xr), np.abs(wr), stride=stride, padding=pad) + np.abs(b8)
    y, S = activate(y, S, act)
    return y, (w4[0].size + 2) * U * S + U


def reference_backward(torch, x, w, d, k, stride, pad, wu0, sd0, rnd_x=bf16_round,
                       rnd_w=bf16_round, rnd_d=bf16_round, swap=False, dtype=np.float64):
    """((ref, bound) of dW, (ref, bound) of dX) in float64 from the rounded
    operands: x [B, C, H, W], w [filters, C*k*k], d [B, filters, oh, ow], and
    the buffers' prior contents.  n = B*oh*ow for dW and filters*k*k for dX."""
    (B, C, H, W), (filters, oh, ow) = x.shape, d.shape[1:]
    xr, dr, wr = rnd_x(x), rnd_d(d), rnd_w(w).reshape(filters, C, k, k)
    if swap:
        wr = wr.transpose(0, 1, 3, 2)

    # dW[f, c] = the correlation of x[:, c] with d[:, f], the batch as channels
    def dw(a, c, dtype=np.float64):
        t = _conv(torch, a.transpose(1, 0, 2, 3), c.transpose(1, 0, 2, 3), dtype, padding=pad,
                  dilation=stride)[:, :, :k, :k].transpose(1, 0, 2, 3)
        return (t.transpose(0, 1, 3, 2) if swap else t).reshape(wu0.shape)

    # dX = d spread by the stride, padded, convolved with the flipped W^T
    def dx(a, c, dtype=np.float64):
        up = np.zeros((B, filters, H + 2 * pad + k - 1, W + 2 * pad + k - 1), dtype)
        up[:, :, k - 1:, k - 1:][:, :, :(oh - 1) * stride + 1:stride,
                                 :(ow - 1) * stride + 1:stride] = a
        full = _conv(torch, up, c.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1], dtype)
        return full[:, :, pad:pad + H, pad:pad + W].reshape(sd0.shape)
    SW, SX = dw(np.abs(xr), np.abs(dr)) + np.abs(wu0), dx(np.abs(dr), np.abs(wr)) + np.abs(sd0)
    return ((dw(xr, dr, dtype) + wu0.astype(dtype), (B * oh * ow + 2) * U * SW + U),
            (dx(dr, wr, dtype) + sd0.astype(dtype), (filters * k * k + 2) * U * SX + U))


def held(got, ref, bound, what):
    """Assert |got - ref| <= bound everywhere; print and return the worst
    error over the bound."""
    err = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
    worst = (err / bound).max()
    print(what, "max err", err.max(), "max err / bound", worst)
    assert (err <= bound).all(), what
    return worst


def _cfg_conv(f, k, s, bn):
    return (f"[convolutional]\nbatch_normalize={bn}\nfilters={f}\nsize={k}\nstride={s}\npad=1\n"
            f"activation={'leaky' if bn else 'linear'}\n")


# A net with branches: conv 2's output goes to conv 3, to the shortcut (layer 4) and to the
# route (layer 7), a maxpool and an upsample sit between convs.  In the backward conv 3's
# input delta already holds the route's and the shortcut's terms when its dX adds to it.
BRANCH_CFG = ("[net]\nbatch=2\nheight=32\nwidth=32\nchannels=3\n" + _cfg_conv(8, 3, 1, 1)
              + "[maxpool]\nsize=2\nstride=2\n" + _cfg_conv(16, 3, 1, 1) + _cfg_conv(16, 1, 1, 0)
              + "[shortcut]\nfrom=-2\nactivation=linear\n" + _cfg_conv(16, 3, 2, 1)
              + "[upsample]\nstride=2\n[route]\nlayers=-1,2\n" + _cfg_conv(16, 3, 1, 0)
              + "[yolo]\nmask=0,1\nnum=2\nclasses=3\nanchors=4,4,8,8\n")
BRANCH_CONVS = [0, 2, 3, 5, 8]
