"""tns_gemm_bf16 / tns_gemm_bf16_nt_packed against a float64 product of the
bf16-rounded operands.

A product of two bf16 values is exact in fp32, so the kernel's only error is
its fp32 accumulation of K products and the prior C, in whatever order and
slice count: with S = |op(A~)| . |op(B~)| + |C0| and U = 2^-23,
|got - ref| <= (K + 2) * U * S + U (tests/_conv_bf16_ref.py).
"""
import numpy as np
import pytest

from _conv_bf16_ref import F, draw, draw_edges, held
from _gemm_bf16_ref import reference

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 4
FORMS = ("NT", "TN", "NN")
GUARD = F(777.0)

# form, M, N, K: the smallest shapes at which the kernel can go wrong
SHAPES = [
    ("NT", 3, 7, 1),       # one k, below every tile
    ("NT", 1, 10, 100),    # the batch-1 inference row; K no multiple of the k step
    ("NT", 33, 65, 40),    # one row and one column past a tile edge; a k tail of 8
    ("TN", 65, 33, 3),     # the lstm dW at three rows; both operands k-slow; K below one MFMA
    ("TN", 40, 24, 1),     # dW at one row
    ("NN", 5, 70, 33),     # B k-slow; k one past the step
] + [(f, 129, 130, 72) for f in FORMS]  # crosses the largest tile both ways; three k stages
# how: plain | shifted (operands one float past a 16-byte boundary, odd leading
# dimensions, guards) | edges (draw_edges data) | packed | split<v> | tile<v> (forced)
CASES = ([(*s, "plain") for s in SHAPES]
         + [(f, 33, 65, 40, how) for f in FORMS for how in ("shifted", "edges", "tile0", "tile1")]
         + [(*s, "packed") for s in SHAPES if s[0] == "NT"]
         + [("NT", 4, 48, 100, "split3"), ("NT", 4, 48, 100, "split1")])


def place(torch, m, shifted, fill=GUARD):
    """m in a guarded device buffer -> (tensor, element offset, ld, mask of m)."""
    rows, cols = m.shape
    off, ld = (5, cols + 1 + cols % 2) if shifted else (0, cols)
    buf, mask = np.full(off + rows * ld + 3, fill, F), np.zeros(off + rows * ld + 3, bool)
    buf[off:off + rows * ld].reshape(rows, ld)[:, :cols] = m
    mask[off:off + rows * ld].reshape(rows, ld)[:, :cols] = True
    return torch.from_numpy(buf).cuda(), off, ld, mask


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_gemm_bf16(hip, torch_cuda, case, acc):
    torch = torch_cuda
    form, M, N, K, how = case
    rng = np.random.default_rng([M, N, K, acc, FORMS.index(form)])
    new = draw_edges if how == "edges" else draw
    a = new(rng, *((K, M) if form == "TN" else (M, K)))
    b = new(rng, *((N, K) if form == "NT" else (K, N)))
    c0 = draw(rng, M, N) if acc else np.zeros((M, N), F)
    ref, bound = reference(form, a, b, c0)
    shifted = how == "shifted"
    (da, oa, lda, _), (db, ob, ldb, _) = place(torch, a, shifted), place(torch, b, shifted)
    # without accumulate C must not be read: NaN there
    dc, oc, ldc, inside = place(torch, c0 if acc else np.full((M, N), np.nan, F), shifted)
    if how == "packed":
        wp = hip.gemmBf16Pack(N, K, db, ob, ldb)
        assert wp.numel() == hip.gemmBf16PackedBytes(N, K)
    hip.setGemmBf16Tile(int(how[4:]) if how.startswith("tile") else -1)
    hip.setGemmBf16Split(int(how[5:]) if how.startswith("split") else -1)
    try:
        outs = []
        for _ in range(2):  # the same call gives the same bits
            c = dc.clone()
            if how == "packed":
                hip.gemmBf16NTPacked(M, N, K, da, oa, lda, wp, acc, c, oc, ldc)
            else:
                hip.gemmBf16(form[0] == "T", form[1] == "T", M, N, K, da, oa, lda, db, ob, ldb,
                             acc, c, oc, ldc)
            hip.finish()
            outs.append(c.cpu().numpy())
    finally:
        hip.setGemmBf16Tile(-1)
        hip.setGemmBf16Split(-1)
    held(outs[0][inside], ref.reshape(-1), bound.reshape(-1), f"{case} accumulate {acc}")
    assert (outs[0][~inside] == GUARD).all(), "a guard element was written"
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.parametrize("what", ["TT", "null A", "null B", "null C", "M = 0", "K = -1", "lda",
                                  "ldb", "ldc", "overlap A", "overlap B", "packed misaligned",
                                  "packed null"])
def test_refusals(hip, torch_cuda, what):
    torch = torch_cuda
    M, N, K = 4, 6, 8
    buf = torch.full((M * K + N * K + M * N,), 7.0, device="cuda")
    A, B, C_ = buf.data_ptr(), buf.data_ptr() + 4 * M * K, buf.data_ptr() + 4 * (M * K + N * K)
    wp = hip.gemmBf16Pack(N, K, buf, M * K)
    v = dict(ta=0, tb=1, M=M, N=N, K=K, A=A, lda=K, B=B, ldb=K, C=C_, ldc=N, wp=wp.data_ptr())
    v.update({"TT": dict(ta=1), "null A": dict(A=None), "null B": dict(B=None),
              "null C": dict(C=None), "M = 0": dict(M=0), "K = -1": dict(K=-1),
              "lda": dict(lda=K - 1), "ldb": dict(ldb=K - 1), "ldc": dict(ldc=N - 1),
              "overlap A": dict(C=A + 4 * (M * K - 1)), "overlap B": dict(C=B - 4 * (M * N - 1)),
              "packed misaligned": dict(wp=wp.data_ptr() + 4), "packed null": dict(wp=None)}[what])
    hip.lib.tns_clear_error()
    if what.startswith("packed"):
        rc = hip.lib.tns_gemm_bf16_nt_packed(hip.ctx, v["M"], v["N"], v["K"], v["A"], v["lda"],
                                             v["wp"], 0, v["C"], v["ldc"])
    else:
        rc = hip.lib.tns_gemm_bf16(hip.ctx, v["ta"], v["tb"], v["M"], v["N"], v["K"], v["A"],
                                   v["lda"], v["B"], v["ldb"], 0, v["C"], v["ldc"])
    assert rc == (ERR_UNSUPPORTED if what == "TT" else ERR_ARG)
    assert hip.lib.tns_last_error() != b""
    hip.lib.tns_clear_error()
    hip.finish()
    assert (buf.cpu().numpy() == 7.0).all()
