"""The side-stream hazard table (test infrastructure, no GPU needed to import).

With TNS_OPT_BWD_OVERLAP = 2 a conv backward leaves its dW product on the side
stream, and every later call joins it only when its operands meet the pending
dW's (check_ops, csrc/tns_ctx.hpp).  This table states, for every tns_hip_*
entry point that takes a context, one small valid call and what each pointer
operand of that call touches: its role and the first and last float index it
touches, relative to the pointer passed.  The extents are written from the
contracts in include/tns.h and from what the NumPy / C oracle of the operation
indexes — a second statement, independent of the library's span(...) lines.

tests/test_hazards.py (CPU) holds the table against the exported ABI and
against the arena; tests/test_gpu_hazards.py places each operand at the edges
of each pending range on the device and compares tns_hip_pending_dw with the
rule.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Callable

# ---- the arena (float indices) ------------------------------------------------
ARENA = 65536                 # floats in the one device tensor
MARGIN = 1024                 # nothing may be touched closer to either end
QUIET = (1024, 16384)         # operands that are not under test live here
HOME = (16384, 18432)         # the pending conv's other operands (weights, output, biases)
GAP = 64                      # between two operands in the quiet region

# the pending dW: the tiny layer of test_softmax_batch_joins_a_pending_dw_it_reads
PB, PC, PH, PF, PK = 2, 4, 8, 4, 3
P_IN = PB * PC * PH * PH              # input
P_OUT = PB * PF * PH * PH             # output / delta ("same" padding)
P_W = PF * PC * PK * PK               # weights / weight_updates
P_COL = PB * PC * PK * PK * PH * PH   # the caller's col workspace


@dataclass(frozen=True)
class Pending:
    name: str
    r0: int        # first float of the range
    r1: int        # last float of the range
    written: bool  # the dW writes it (weight_updates, col); else it reads it


PENDING = (
    Pending("delta", 24576, 24576 + P_OUT - 1, False),
    Pending("input", 32768, 32768 + P_IN - 1, False),
    Pending("weight_updates", 40960, 40960 + P_W - 1, True),
    Pending("col", 49152, 49152 + P_COL - 1, True),
)
HOME_WEIGHTS = HOME[0]
HOME_OUTPUT = HOME[0] + 256
HOME_BIAS_UPDATES = HOME[0] + 1024

# 1: ends just below R; 2: last element is R's first; 3: first element is R's
# last; 4: starts just above R
PLACEMENTS = (1, 2, 3, 4)


@dataclass(frozen=True)
class Op:
    """One pointer operand.  role: "r" read, "w" written, "rw" both (in-place
    or accumulated into), "side" an operand the call hands to the side stream
    itself (a pipelined conv backward's dW operands: queued behind the pending
    dW, never a reason to join).  first / last: the touched float indices
    relative to the pointer passed (an int64 element counts as two floats).
    claim: where the library's declared range is pinned wider than what is
    touched, that range, with `why`.  null: passed as NULL.  zero: zeroed
    before the call (int64 operands a kernel reads)."""
    name: str
    role: str
    first: int = 0
    last: int = 0
    i64: bool = False
    claim: tuple | None = None
    why: str = ""
    null: bool = False
    zero: bool = False

    @property
    def extent(self):
        """What the join decision is expected to see."""
        return self.claim if self.claim else (self.first, self.last)

    @property
    def hull(self):
        """Everything touched or claimed (arena bounds)."""
        f, l = self.extent
        return min(f, self.first), max(l, self.last)


@dataclass(frozen=True)
class Case:
    id: str
    sym: str
    ops: tuple
    args: Callable        # SimpleNamespace of pointers (int or None) -> argument list after ctx
    adds_pending: int = 0  # dW products the call itself queues (a second conv backward)


def R(name, first, last, **kw):
    return Op(name, "r", first, last, **kw)


def W(name, first, last, **kw):
    return Op(name, "w", first, last, **kw)


def RW(name, first, last, **kw):
    return Op(name, "rw", first, last, **kw)


def NULL(name, role="r"):
    return Op(name, role, null=True)


LEAKY, LINEAR, LOGISTIC, TANH = 9, 4, 0, 6
CASES: list[Case] = []


def case(id, sym, ops, args, **kw):
    assert all(c.id != id for c in CASES), id
    CASES.append(Case(id, sym, tuple(ops), args, **kw))


# ---- GEMM ---------------------------------------------------------------------
# C (M x N, ldc) = alpha * op(A) . op(B) + beta * C; op(A) is M x K: A is M x K
# (lda >= K) or, transposed, K x M (lda >= M); a matrix of rows x cols with
# leading dimension ld ends at (rows - 1) * ld + cols - 1
def _mat(off, rows, cols, ld, stride=0, batch=1):
    return off, off + (batch - 1) * stride + (rows - 1) * ld + cols - 1


_M, _N, _K = 3, 5, 4
case("gemm-nn-ld-offsets", "tns_hip_gemm",
     [R("A", *_mat(2, _M, _K, 6)), R("B", *_mat(1, _K, _N, 7)), RW("C", *_mat(3, _M, _N, 8))],
     lambda p: [0, 0, _M, _N, _K, 1.0, p.A, 2, 6, p.B, 1, 7, 1.0, p.C, 3, 8])
case("gemm-tt-ld-offsets", "tns_hip_gemm",
     [R("A", *_mat(2, _K, _M, 5)), R("B", *_mat(1, _N, _K, 6)), RW("C", *_mat(3, _M, _N, 8))],
     lambda p: [1, 1, _M, _N, _K, 1.0, p.A, 2, 5, p.B, 1, 6, 0.5, p.C, 3, 8])
# strideA = 0 shares A (the conv weights); B and C: stride > one matrix's span
case("gemm-strided-batched", "tns_hip_gemm_strided_batched",
     [R("A", *_mat(2, _M, _K, 6)), R("B", *_mat(1, _K, _N, 7, 40, 3)),
      RW("C", *_mat(3, _M, _N, 8, 30, 3))],
     lambda p: [0, 0, _M, _N, _K, 1.0, p.A, 2, 6, 0, p.B, 1, 7, 40, 1.0, p.C, 3, 8, 30, 3])
case("gemm-strided-batched-nt", "tns_hip_gemm_strided_batched",
     [R("A", *_mat(0, _M, _K, 4, 12, 2)), R("B", *_mat(5, _N, _K, 6, 33, 2)),
      RW("C", *_mat(0, _M, _N, 5, 15, 2))],
     lambda p: [0, 1, _M, _N, _K, 1.0, p.A, 0, 4, 12, p.B, 5, 6, 33, 0.0, p.C, 0, 5, 15, 2])
# a negative batch stride puts GEMM b at b*stride below the pointer: the
# operand starts (batch - 1)*|stride| below it and ends with GEMM 0's matrix
case("gemm-strided-batched-negative-stride", "tns_hip_gemm_strided_batched",
     [R("A", *_mat(2, _M, _K, 6)), R("B", 1 - 2 * 40, _mat(1, _K, _N, 7)[1]),
      RW("C", 3 - 2 * 32, _mat(3, _M, _N, 8)[1])],
     lambda p: [0, 0, _M, _N, _K, 1.0, p.A, 2, 6, 0, p.B, 1, 7, -40, 1.0, p.C, 3, 8, -32, 3])

# ---- im2col / col2im -----------------------------------------------------------
# 2 channels, 5 x 5, 3 x 3 window, pad 1, stride 1: 5 x 5 columns; an image is
# C*H*W floats, its col matrix C*kH*kW*oh*ow, every element of either touched
_IC, _IH, _IK = 2, 5, 3
_IM, _COL = _IC * _IH * _IH, _IC * _IK * _IK * _IH * _IH
_geo = [_IC, _IH, _IH, _IK, _IK, 1, 1, 1, 1, 1, 1]
case("im2col", "tns_hip_im2col",
     [R("im", 3, 3 + _IM - 1), W("col", 5, 5 + _COL - 1)],
     lambda p: [*_geo, p.im, 3, p.col, 5])
case("im2col-strided-batched", "tns_hip_im2col_strided_batched",
     [R("im", 3, 3 + 60 + _IM - 1), W("col", 5, 5 + 500 + _COL - 1)],
     lambda p: [*_geo, p.im, 60, 3, p.col, 500, 5, 2])
case("col2im", "tns_hip_col2im",
     [R("col", 5, 5 + _COL - 1), RW("im", 3, 3 + _IM - 1)],
     lambda p: [*_geo, p.col, 5, p.im, 3])
case("col2im-strided-batched", "tns_hip_col2im_strided_batched",
     [R("col", 5, 5 + 500 + _COL - 1), RW("im", 3, 3 + 60 + _IM - 1)],
     lambda p: [*_geo, p.col, 500, 5, p.im, 60, 3, 2])

# ---- bias, activation -----------------------------------------------------------
# dst[(b*srcSize + i)*bs + j] += src[i*incb]: batch 2, srcSize 3, bs 4
case("forward-bias-incb", "tns_hip_forward_bias",
     [RW("dst", 5, 5 + 23), R("src", 0, 2 * 2)],
     lambda p: [24, p.dst, 5, 3, p.src, 2, 2])
# dst[i*incb] += sum_b sum_j src[(b*dstSize + i)*bs + j]
case("backward-bias-incb", "tns_hip_backward_bias",
     [RW("dst", 0, 2 * 2), R("src", 5, 5 + 23)],
     lambda p: [3, p.dst, 24, p.src, 5, 2, 2])
case("backward-bias-fc", "tns_hip_backward_bias",       # bs == 1: the FC layers' sum
     [RW("dst", 0, 2), R("src", 1, 1 + 11)],
     lambda p: [3, p.dst, 12, p.src, 1, 1, 4])
case("backward-bias-conv-blocks", "tns_hip_backward_bias",   # bs >= 64: the block chains
     [RW("dst", 0, 2), R("src", 2, 2 + 2 * 3 * 64 - 1)],
     lambda p: [3, p.dst, 2 * 3 * 64, p.src, 2, 1, 2])
case("activate", "tns_hip_activate_array", [RW("x", 3, 3 + 15)],
     lambda p: [16, p.x, 3, LEAKY])
case("derive", "tns_hip_derive_array", [R("x", 3, 3 + 15), RW("delta", 0, 15)],
     lambda p: [16, p.x, 3, LEAKY, p.delta])

# ---- BLAS-1 ---------------------------------------------------------------------
case("axpy-inc", "tns_hip_axpy", [R("x", 1, 1 + 7 * 2), RW("y", 2, 2 + 7 * 3)],
     lambda p: [8, 0.5, p.x, 1, 2, p.y, 2, 3])
case("axpy-broadcast", "tns_hip_axpy",
     [R("x", 1, 1, claim=(1, 1 + 7), why="inc == 0 keeps span()'s conservative n-element claim"),
      RW("y", 0, 7)],
     lambda p: [8, 0.5, p.x, 1, 0, p.y, 0, 1])
_sgd = lambda p: [20, p.weights, p.weight_updates, 4, p.biases, p.bias_updates, p.scales,
                  p.scale_updates, 0.01, -0.001, 0.9]
case("sgd-update", "tns_hip_sgd_update",
     [RW("weights", 0, 19), RW("weight_updates", 0, 19), RW("biases", 0, 3),
      RW("bias_updates", 0, 3), RW("scales", 0, 3), RW("scale_updates", 0, 3)], _sgd)
case("sgd-update-no-scales", "tns_hip_sgd_update",
     [RW("weights", 0, 19), RW("weight_updates", 0, 19), RW("biases", 0, 3),
      RW("bias_updates", 0, 3), NULL("scales", "rw"), NULL("scale_updates", "rw")], _sgd)
case("scale-stride", "tns_hip_scale", [RW("x", 0, 7 * 3)], lambda p: [8, 0.5, p.x, 3])
case("fill-offset-stride", "tns_hip_fill", [W("x", 2, 2 + 7 * 3)],
     lambda p: [8, p.x, 2, 0.25, 3])
case("copy-inc", "tns_hip_copy", [R("src", 1, 1 + 7 * 2), W("dst", 2, 2 + 7 * 3)],
     lambda p: [8, p.src, 1, 2, p.dst, 2, 3])
case("copy-broadcast", "tns_hip_copy",
     [R("src", 4, 4, claim=(4, 4 + 7), why="inc == 0 keeps span()'s conservative n-element claim"),
      W("dst", 0, 7)],
     lambda p: [8, p.src, 4, 0, p.dst, 0, 1])
case("clamp-stride-offset", "tns_hip_clamp", [R("src", 3, 3 + 7 * 2), W("dst", 3, 3 + 7 * 2)],
     lambda p: [8, 1.0, p.src, p.dst, 2, 3])
case("clamp-in-place", "tns_hip_clamp", [RW("x", 3, 3 + 7 * 2)],
     lambda p: [8, 1.0, p.x, p.x, 2, 3])

# ---- TNNCuda vector ops: dst[i*incc] = src1[i*inca] op src2[i*incb] ---------------
for _name in ("addvv", "subvv", "mulvv"):
    case(f"{_name}-inc", f"tns_hip_{_name}",
         [R("a", 5, 5 + 7 * 3), R("b", 3, 3 + 7 * 2), W("d", 1, 1 + 7 * 2)],
         lambda p: [8, p.a, 5, 3, p.b, 3, 2, p.d, 1, 2])
    # negative increments walk downward: the pointer (+ offset) is the highest
    # element touched, element i at i*inc below it
    case(f"{_name}-negative-inc", f"tns_hip_{_name}",
         [R("a", 2 - 7 * 1, 2), R("b", -7 * 2, 0), W("d", 1 - 7 * 3, 1)],
         lambda p: [8, p.a, 2, -1, p.b, 0, -2, p.d, 1, -3])
case("addvv-in-place", "tns_hip_addvv", [RW("a", 0, 15), R("b", 0, 15)],
     lambda p: [16, p.a, 0, 1, p.b, 0, 1, p.a, 0, 1])
case("addvv-broadcast", "tns_hip_addvv",
     [R("a", 0, 7), R("b", 2, 2, claim=(2, 2 + 7),
                      why="inc == 0 keeps span()'s conservative n-element claim"), W("d", 0, 7)],
     lambda p: [8, p.a, 0, 1, p.b, 2, 0, p.d, 0, 1])
case("fmavv-inc", "tns_hip_fmavv",
     [R("a", 5, 5 + 7 * 3), R("b", 3, 3 + 7 * 2), R("c", 7, 7 + 7), W("d", 2, 2 + 7 * 2)],
     lambda p: [8, p.a, 5, 3, p.b, 3, 2, p.c, 7, 1, p.d, 2, 2])
case("fmavv-negative-inc", "tns_hip_fmavv",
     [R("a", -7 * 2, 0), R("b", 1 - 7, 1), R("c", 3 - 7 * 3, 3), W("d", -7, 0)],
     lambda p: [8, p.a, 0, -2, p.b, 1, -1, p.c, 3, -3, p.d, 0, -1])
case("fmavss", "tns_hip_fmavss", [R("src", 3, 3 + 15), W("dst", 3, 3 + 15)],
     lambda p: [16, p.src, 3, 1.5, -0.25, p.dst])
case("inverse-sqrt-stride", "tns_hip_inverse_sqrt", [R("src", 3, 3 + 7 * 2), W("dst", 3, 3 + 7 * 2)],
     lambda p: [8, 0.0, p.src, p.dst, 2, 3])

# ---- the non-convolutional YOLOv3 layers ---------------------------------------
case("shortcut", "tns_hip_shortcut", [R("a", 1, 16), R("b", 2, 17), W("out", 3, 18)],
     lambda p: [16, p.a, 1, p.b, 2, p.out, 3, LEAKY])
# planes = 1*2, the small tensor 3 x 3, stride 2: small 18 floats, big 72.
# Forward reads the small one and writes the big one; backward adds into the
# small one what it reads from the big one
case("upsample-forward", "tns_hip_upsample", [R("in_", 0, 17), W("out", 0, 71)],
     lambda p: [1, 2, 3, 3, p.in_, 2, 1, 1.0, p.out, 0])
case("upsample-backward", "tns_hip_upsample", [RW("in_", 0, 17), R("out", 0, 71)],
     lambda p: [1, 2, 3, 3, p.in_, 2, 0, 1.0, p.out, 0])
case("upsample-backward-zero-in", "tns_hip_upsample", [W("in_", 0, 17), R("out", 0, 71)],
     lambda p: [1, 2, 3, 3, p.in_, 2, 0, 1.0, p.out, 1])
# data [batch][anchors][classes + 5][hw]
_YN = 1 * 2 * (1 + 5) * 4
case("yolo-forward", "tns_hip_yolo_forward", [R("in_", 0, _YN - 1), W("out", 0, _YN - 1)],
     lambda p: [1, 2, 1, 4, p.in_, p.out])
case("yolo-forward-in-place", "tns_hip_yolo_forward", [RW("x", 0, _YN - 1)],
     lambda p: [1, 2, 1, 4, p.x, p.x])


def _host(ctype, *vals):
    return (ctype * len(vals))(*vals)


# batch 1, one anchor of one, one class, 2 x 2 cells: output / delta 24 floats;
# truth [batch][maxBoxes = 2][6] (every row is loaded); cost[0]; stats[2*batch];
# counters int64[2]; mask and biases are host arrays
def _yolo_loss(p):
    return [1, 1, 1, 2, 2, 1, _host(C.c_int64, 0), _host(C.c_float, 1.0, 1.0), 2, 32, 32,
            0.7, 1.0, 1.0, 0.75, 1.0, p.output, p.truth, p.delta, p.cost, p.stats, p.counters]


_yl = [RW("output", 0, 23), R("truth", 0, 11, zero=True), W("delta", 0, 23), W("cost", 0, 0)]
case("yolo-loss", "tns_hip_yolo_loss",
     _yl + [W("stats", 0, 1), RW("counters", 0, 3, i64=True, zero=True)], _yolo_loss)
case("yolo-loss-no-stats", "tns_hip_yolo_loss",
     _yl + [NULL("stats", "w"), RW("counters", 0, 3, i64=True, zero=True)], _yolo_loss)
# two images of the output above; capacity 4: counts int64[batch], boxes
# [batch][4][4], objectness [batch][4], probs [batch][4][classes].  Only the
# taken rows are written: the claim is the buffer the contract names
_rows = "rows are taken by the data: the claim is the whole buffer of the contract"
case("yolo-detections", "tns_hip_yolo_detections",
     [R("output", 0, 47), RW("counts", 0, 3, i64=True, zero=True), W("boxes", 0, 31, why=_rows),
      W("objectness", 0, 7, why=_rows), W("probs", 0, 7, why=_rows)],
     lambda p: [2, 1, 1, 2, 2, 1, _host(C.c_int64, 0), _host(C.c_float, 1.0, 1.0), 32, 32, 64, 48,
                0.5, 1, 0, p.output, 4, p.counts, p.boxes, p.objectness, p.probs])
case("nms-sort", "tns_hip_nms_sort",
     [R("counts", 0, 3, i64=True, zero=True), R("boxes", 0, 31, why=_rows),
      R("objectness", 0, 7, why=_rows), RW("probs", 0, 15, why=_rows)],
     lambda p: [2, 4, 2, p.counts, p.boxes, p.objectness, p.probs, 0.45])

# ---- pooling: [1][2][4][4] -> [1][2][2][2], window 2, stride 2 ---------------------
_pool_f = lambda p: [1, 2, 2, 2, p.input, 2, 4, 4, 2, 2, 0, 2]
_pool_b = lambda p: [4, 4, 2, 2, 0, 2]
case("maxpool-forward", "tns_hip_maxpool_forward",
     [R("input", 0, 31), W("indexes", 0, 15, i64=True), W("output", 0, 7)],
     lambda p: [*_pool_f(p), p.indexes, p.output])
case("maxpool-forward-no-indexes", "tns_hip_maxpool_forward",
     [R("input", 0, 31), NULL("indexes", "w"), W("output", 0, 7)],
     lambda p: [*_pool_f(p), p.indexes, p.output])
case("maxpool-backward", "tns_hip_maxpool_backward",
     [RW("output", 0, 31, why="only named elements are written: the claim is the whole delta"),
      R("indexes", 0, 15, i64=True, zero=True), R("delta", 0, 7)],
     lambda p: [1, 2, 2, 2, p.output, p.indexes, p.delta, *_pool_b(p)])
case("avgpool-forward", "tns_hip_avgpool_forward", [R("input", 0, 31), W("output", 0, 7)],
     lambda p: [*_pool_f(p), p.output])
case("avgpool-backward", "tns_hip_avgpool_backward", [RW("output", 0, 31), R("delta", 0, 7)],
     lambda p: [1, 2, 2, 2, p.output, p.delta, *_pool_b(p)])

# ---- dropout, loss heads ---------------------------------------------------------
case("dropout-forward", "tns_hip_dropout_forward",
     [R("src", 0, 15), W("rnd", 0, 15), W("dst", 0, 15)],
     lambda p: [16, 7, 0.5, 2.0, p.src, p.rnd, p.dst])
case("dropout-forward-in-place", "tns_hip_dropout_forward", [RW("x", 0, 15), W("rnd", 0, 15)],
     lambda p: [16, 7, 0.5, 2.0, p.x, p.rnd, p.x])
case("dropout-backward", "tns_hip_dropout_backward",
     [R("src", 0, 15), R("rnd", 0, 15), W("dst", 0, 15)],
     lambda p: [16, 0.5, 2.0, p.src, p.rnd, p.dst])
case("dropout-backward-in-place", "tns_hip_dropout_backward", [RW("x", 0, 15), R("rnd", 0, 15)],
     lambda p: [16, 0.5, 2.0, p.x, p.rnd, p.x])
_heads = [R("pred", 0, 15), R("truth", 0, 15), W("delta", 0, 15), W("error", 0, 15)]
_heads_args = lambda p: [16, p.pred, p.truth, p.delta, p.error]
case("cost-l2", "tns_hip_cost_l2", _heads, _heads_args)
case("cross-entropy-logistic", "tns_hip_cross_entropy_logistic", _heads, _heads_args)
case("cross-entropy-softmax", "tns_hip_cross_entropy_softmax", _heads, _heads_args)

# ---- LSTM / RNN step stages (N floats per operand, the biases H) --------------------
_gates = ["wf", "wi", "wg", "wo", "uf", "ui", "ug", "uo"]
_g8 = [R(n, 0, 7) for n in _gates]
case("lstm-gates-forward", "tns_hip_lstm_gates_forward",
     _g8 + [RW("c_state", 0, 7), W("h_state", 0, 7), W("cell_slice", 0, 7), W("out_slice", 0, 7)],
     lambda p: [8, *[getattr(p, n) for n in _gates], p.c_state, p.h_state, p.cell_slice,
                p.out_slice])
_lb_in = _g8 + [R("cell_i", 0, 7), R("cprev", 0, 7), R("delta_i", 0, 7)]
_lb_dw, _lb_du = ["dwf", "dwi", "dwg", "dwo"], ["duf", "dui", "dug", "duo"]
_lb_args = lambda p: [8, *[getattr(p, n) for n in _gates], p.cell_i, p.cprev, p.delta_i, p.dc,
                      *[getattr(p, n) for n in _lb_dw + _lb_du]]
case("lstm-gates-backward", "tns_hip_lstm_gates_backward",
     _lb_in + [RW("dc", 0, 7)] + [W(n, 0, 7) for n in _lb_dw + _lb_du], _lb_args)
case("lstm-gates-backward-no-du", "tns_hip_lstm_gates_backward",
     _lb_in + [RW("dc", 0, 7)] + [W(n, 0, 7) for n in _lb_dw] + [NULL(n, "w") for n in _lb_du],
     _lb_args)
_rnn_f = lambda p: [8, 4, p.in_slice, p.in_bias, LEAKY, p.self_slice, p.self_bias, TANH,
                    p.state_prev, p.state_next]
case("rnn-state-forward", "tns_hip_rnn_state_forward",
     [RW("in_slice", 0, 7), R("in_bias", 0, 3), RW("self_slice", 0, 7), R("self_bias", 0, 3),
      R("state_prev", 0, 7), W("state_next", 0, 7)], _rnn_f)
case("rnn-state-forward-no-bias-no-prev", "tns_hip_rnn_state_forward",
     [RW("in_slice", 0, 7), NULL("in_bias"), RW("self_slice", 0, 7), NULL("self_bias"),
      NULL("state_prev"), W("state_next", 0, 7)], _rnn_f)
case("rnn-state-forward-in-place", "tns_hip_rnn_state_forward",
     [RW("in_slice", 0, 7), R("in_bias", 0, 3), RW("self_slice", 0, 7), R("self_bias", 0, 3),
      RW("state", 0, 7)],
     lambda p: [8, 4, p.in_slice, p.in_bias, LEAKY, p.self_slice, p.self_bias, TANH, p.state,
                p.state])
_rnn_b = lambda p: [8, p.delta, p.out, LEAKY, p.delta2, p.out2, TANH]
case("rnn-delta-backward", "tns_hip_rnn_delta_backward",
     [RW("delta", 0, 7), R("out", 0, 7), W("delta2", 0, 7), R("out2", 0, 7)], _rnn_b)
case("rnn-delta-backward-one-slice", "tns_hip_rnn_delta_backward",
     [RW("delta", 0, 7), R("out", 0, 7), NULL("delta2", "w"), NULL("out2")], _rnn_b)

# ---- batch norm: data [groups = 2][channels = 3][blockSize = 4] at an offset ----------
_BN, _BC, _BG, _BO = 24, 3, 2, 5
_data = (_BO, _BO + _BN - 1)
case("means-and-vars", "tns_hip_means_and_vars",
     [R("src", *_data), W("means", 0, 2), W("vars", 0, 2)],
     lambda p: [_BN, _BC, _BG, p.src, _BO, p.means, p.vars])
case("means", "tns_hip_means", [R("src", *_data), W("means", 0, 2)],
     lambda p: [_BN, _BC, _BG, p.src, _BO, p.means])
case("variances", "tns_hip_variances", [R("src", *_data), R("means", 0, 2), W("vars", 0, 2)],
     lambda p: [_BN, _BC, _BG, p.src, _BO, p.means, p.vars])
# channel i's statistics at means[i*meansStride], vars[i*varsStride]
case("normalize-strides", "tns_hip_normalize",
     [R("means", 0, 2 * 2), R("vars", 0, 2 * 3), RW("dst", *_data)],
     lambda p: [_BC, _BN, _BG, p.means, 2, p.vars, 3, p.dst, _BO])
case("forward-scale-incb", "tns_hip_forward_scale", [RW("dst", *_data), R("scale", 0, 2 * 2)],
     lambda p: [_BN, p.dst, _BO, _BC, p.scale, 2, _BG])
case("forward-scale-add-incb", "tns_hip_forward_scale_add",
     [RW("dst", *_data), R("scales", 0, 2 * 2), R("biases", 0, 2 * 2)],
     lambda p: [_BN, p.dst, _BO, _BC, p.scales, p.biases, 2, _BG])
case("forward-scale-add-no-biases", "tns_hip_forward_scale_add",
     [RW("dst", *_data), R("scales", 0, 2), NULL("biases")],
     lambda p: [_BN, p.dst, _BO, _BC, p.scales, p.biases, 1, _BG])
case("means-and-vars-delta", "tns_hip_means_and_vars_delta",
     [R("delta", *_data), R("x", *_data), R("mean", 0, 2), R("variance", 0, 2),
      W("mean_delta", 0, 2), W("variance_delta", 0, 2)],
     lambda p: [_BN, _BC, _BG, p.delta, p.x, _BO, p.mean, p.variance, p.mean_delta,
                p.variance_delta])
case("normalize-delta", "tns_hip_normalize_delta",
     [RW("delta", *_data), R("x", *_data), R("mean", 0, 2), R("variance", 0, 2),
      R("mean_delta", 0, 2), R("variance_delta", 0, 2)],
     lambda p: [_BN, _BC, _BG, p.delta, p.x, _BO, p.mean, p.variance, p.mean_delta,
                p.variance_delta])
case("add-dots", "tns_hip_add_dots", [R("src1", *_data), R("src2", *_data), RW("dst", 0, 2)],
     lambda p: [_BN, _BC, _BG, p.src1, p.src2, _BO, p.dst])
# rows of N = 4 elements every 3, row (b, g) at b*40 + g*12: the last row's
# last element ends the extent
_SM = 1 * 40 + 1 * 12 + 3 * 3
case("softmax-batch-rows", "tns_hip_softmax_batch",
     [R("input", 2, 2 + _SM), W("output", 1, 1 + _SM)],
     lambda p: [4, p.input, 2, 2, 40, 2, 12, 3, 1.0, p.output, 1])
case("sum", "tns_hip_sum", [R("src", 3, 3 + 15), W("out", 0, 0)],
     lambda p: [16, p.src, 3, p.out])

# ---- a second pipelined conv backward ---------------------------------------------
# batch 1, 2 channels, 4 x 4, 2 filters, 3 x 3, pad 1.  On the context's stream
# it derives delta in place from output, adds into bias_updates (or the batch
# norm's updates) and runs state.delta's chain from weights and delta; its own
# dW (input, weight_updates, the workspace's col matrix) queues on the side
# stream behind the pending one and is no reason to join
_c_in, _c_w, _c_out, _c_col = 1 * 2 * 16, 2 * 2 * 9, 1 * 2 * 16, 1 * 2 * 9 * 16
_conv_shape = [1, 2, 4, 4]
_side = [Op("input", "side", 0, _c_in - 1), Op("weight_updates", "side", 0, _c_w - 1),
         Op("workspace", "side", 0, _c_col - 1)]
case("conv-backward-second", "tns_hip_conv_backward",
     [R("weights", 0, _c_w - 1), R("output", 0, _c_out - 1), RW("delta", 0, _c_out - 1),
      RW("bias_updates", 0, 1), RW("state_delta", 0, _c_in - 1)] + _side,
     lambda p: [*_conv_shape, p.input, p.weights, 2, 3, 1, 1, 1, LEAKY, p.output, p.delta,
                p.bias_updates, p.weight_updates, p.workspace, p.state_delta],
     adds_pending=1)
case("conv-backward-second-no-state-delta", "tns_hip_conv_backward",
     [R("weights", 0, _c_w - 1, claim=(0, _c_w - 1),
        why="without a state.delta nothing on the context's stream reads the weights; the "
            "claim does not depend on state_delta"),
      R("output", 0, _c_out - 1), RW("delta", 0, _c_out - 1),
      RW("bias_updates", 0, 1), NULL("state_delta", "rw")] + _side,
     lambda p: [*_conv_shape, p.input, p.weights, 2, 3, 1, 1, 1, LEAKY, p.output, p.delta,
                p.bias_updates, p.weight_updates, p.workspace, p.state_delta],
     adds_pending=1)
case("conv-backward-bn-second", "tns_hip_conv_backward_bn",
     [R("weights", 0, _c_w - 1), R("output", 0, _c_out - 1), RW("delta", 0, _c_out - 1),
      R("scales", 0, 1), R("x", 0, _c_out - 1), R("x_norm", 0, _c_out - 1), R("mean", 0, 1),
      R("variance", 0, 1), RW("scale_updates", 0, 1), W("mean_delta", 0, 1),
      W("variance_delta", 0, 1), RW("state_delta", 0, _c_in - 1)] + _side,
     lambda p: [*_conv_shape, p.input, p.weights, 2, 3, 1, 1, 1, LEAKY, p.output, p.delta,
                p.scales, p.x, p.x_norm, p.mean, p.variance, p.scale_updates, p.mean_delta,
                p.variance_delta, p.weight_updates, p.workspace, p.state_delta],
     adds_pending=1)

# ---- entry points that always join (check_ctx): one call each, operands in the
# quiet region; `ops` only states what the call touches, for the arena check ----------
ALWAYS: list[Case] = []
MLP_WIDTHS, MLP_ACTS, MLP_BATCH = (7, 5, 3), (1, LINEAR), 3
MLP_BUF_BOUND = 2048   # >= tns_mlp_buffer_floats(...) (held against the library on the device)


def always(id, sym, ops, args):
    assert all(c.id != id for c in ALWAYS), id
    ALWAYS.append(Case(id, sym, tuple(ops), args))


_fwd_ops = [R("input", 0, _c_in - 1), R("weights", 0, _c_w - 1), W("workspace", 0, _c_col - 1),
            W("out", 0, _c_out - 1)]
always("finish", "tns_hip_finish", [], lambda p: [])
always("set-stream", "tns_hip_set_stream", [], lambda p: [p.stream])
always("get-stream", "tns_hip_get_stream", [], lambda p: [])
always("malloc-free", "tns_hip_malloc", [], None)     # (the device test frees what it got)
always("free", "tns_hip_free", [], None)
always("write-buffer", "tns_hip_write_buffer", [W("dev", 0, 7)],
       lambda p: [p.dev, 32, _host(C.c_float, *[0.5] * 8)])
always("read-buffer", "tns_hip_read_buffer", [R("dev", 0, 7)],
       lambda p: [p.dev, 32, _host(C.c_float, *[0.0] * 8)])
always("gemm-batched", "tns_hip_gemm_batched",
       [R("A", 0, 2 * 12 - 1), R("B", 0, 2 * 20 - 1), RW("C", 0, 2 * 15 - 1)],
       lambda p: [0, 0, _M, _N, _K, 1.0, _host(C.c_void_p, p.A, p.A + 4 * 12), 0, _K,
                  _host(C.c_void_p, p.B, p.B + 4 * 20), 0, _N, 1.0,
                  _host(C.c_void_p, p.C, p.C + 4 * 15), 0, _N, 2])
always("gemm-variant", "tns_hip_gemm_variant",
       [R("A", 0, 11), R("B", 0, 19), RW("C", 0, 14)],
       lambda p: [-1, 0, 0, _M, _N, _K, 1.0, p.A, 0, _K, 0, p.B, 0, _N, 0, 1.0, p.C, 0, _N, 0, 1])
always("mlp-train-step", "tns_hip_mlp_train_step",
       [R("X", 0, MLP_BATCH * MLP_WIDTHS[0] - 1), R("truth", 0, MLP_BATCH * MLP_WIDTHS[-1] - 1),
        RW("buf", 0, MLP_BUF_BOUND - 1), W("cost", 0, 0)],
       lambda p: [len(MLP_ACTS), _host(C.c_int64, *MLP_WIDTHS), _host(C.c_int32, *MLP_ACTS), 0,
                  MLP_BATCH, p.X, p.truth, 0.01, 0.9, 0.0005, p.buf, p.cost])
always("conv2d", "tns_hip_conv2d", _fwd_ops,
       lambda p: [*_conv_shape, p.input, p.weights, 2, 3, 3, 1, 1, 1, 1, 1, 1, p.workspace, p.out])
always("conv-forward", "tns_hip_conv_forward", _fwd_ops + [R("biases", 0, 1)],
       lambda p: [*_conv_shape, p.input, p.weights, p.biases, 2, 3, 1, 1, 1, LEAKY, p.workspace,
                  p.out, 0])
always("conv-forward-train", "tns_hip_conv_forward_train",
       _fwd_ops + [R("scales", 0, 1), R("biases", 0, 1), RW("rolling_mean", 0, 1),
                   RW("rolling_variance", 0, 1), W("mean", 0, 1), W("variance", 0, 1),
                   W("x", 0, _c_out - 1), W("x_norm", 0, _c_out - 1)],
       lambda p: [*_conv_shape, p.input, p.weights, 2, 3, 1, 1, 1, LEAKY, p.scales, p.biases,
                  p.rolling_mean, p.rolling_variance, 0.1, 1, p.mean, p.variance, p.x, p.x_norm,
                  p.workspace, p.out])
always("set-telemetry", "tns_hip_set_telemetry", [], lambda p: [0])

# ---- the classification of every exported tns_hip_* name ---------------------------
TABLE_SYMBOLS = {c.sym for c in CASES}
ALWAYS_JOINS = {c.sym for c in ALWAYS}
NEVER_JOINS = {"tns_hip_pending_dw", "tns_hip_op_ms"}     # pure getters
NO_CONTEXT = {
    "tns_hip_create",                        # makes the context
    "tns_hip_destroy",                       # ends it (drains every stream): nothing follows
    "tns_hip_sgemm_strided_batched_multi",   # host pointers, pool contexts of its own
}


# ---- placement ----------------------------------------------------------------------
def expected_join(op: Op, rng: Pending, placement: int) -> bool:
    """The rule of check_ops: a call joins iff it writes a range the pending
    dW reads or writes, or reads one the dW writes.  Placements 2 and 3 share
    one element with R; 1 and 4 share none."""
    if placement in (1, 4) or op.role == "side":
        return False
    return "w" in op.role or rng.written


def layout(c: Case, x: Op | None = None, rng: Pending | None = None, placement: int = 0) -> dict:
    """Pointer position (float index into the arena) of every operand: x at
    `placement` against rng, every other operand packed into the quiet
    region.  An int64 operand sits on an even index (8-byte aligned: the
    ranges start on even indices and end on odd ones) and shares a whole int64
    with R in placements 2 and 3."""
    pos, cursor = {}, QUIET[0]
    for op in c.ops:
        if op.null:
            pos[op.name] = None
            continue
        # (every operand keeps its quiet slot, so the others do not move when
        # one of them is taken out to a pending range)
        lo, hi = op.hull
        cursor = (cursor + 15) // 16 * 16
        at = cursor - lo
        if op.i64 and at % 2:
            at += 1
        pos[op.name] = at
        cursor = at + hi + 1 + GAP
        if x is not None and op.name == x.name:
            f, l = op.extent
            step = 2 if op.i64 else 1
            pos[op.name] = {1: rng.r0 - 1 - l, 2: rng.r0 + step - 1 - l,
                            3: rng.r1 - step + 1 - f, 4: rng.r1 + 1 - f}[placement]
    return pos


def touched(c: Case, pos: dict) -> dict:
    """name -> (first, last) absolute float indices touched or claimed."""
    return {op.name: (pos[op.name] + op.hull[0], pos[op.name] + op.hull[1])
            for op in c.ops if not op.null}


def pointers(c: Case, pos: dict, base: int, **extra) -> SimpleNamespace:
    """The argument namespace for c.args: addresses from arena positions."""
    return SimpleNamespace(**{n: (None if at is None else base + 4 * at) for n, at in pos.items()},
                           **extra)


def trials(c: Case):
    """Every (operand, pending range, placement) of a case."""
    for op in c.ops:
        if op.null:
            continue
        for rng in PENDING:
            for placement in PLACEMENTS:
                yield op, rng, placement
