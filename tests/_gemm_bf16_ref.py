"""The float64 reference and the derived bound of the bf16 GEMM tests."""
import numpy as np

from _conv_bf16_ref import U, bf16_round


def reference(form, a, b, c0):
    """(ref, bound) of op(a~) . op(b~) + c0 from a [M][K] ([K][M] for TN) and b
    [K][N] ([N][K] for NT): S = |op(a~)| . |op(b~)| + |c0|, bound (K + 2) U S + U."""
    A, B = bf16_round(a).astype(np.float64), bf16_round(b).astype(np.float64)
    A, B = (A.T if form == "TN" else A), (B.T if form == "NT" else B)
    S = np.abs(A) @ np.abs(B) + np.abs(c0)
    return A @ B + c0, (A.shape[1] + 2) * U * S + U
