"""The bf16 convolution tests' own references and data (tests/_conv_bf16_ref.py),
checked without a GPU: the references against autograd, the edge data's
composition, and that on this data the derived bound tells a wrong operand
rounding or a transposed kernel from the right one — so a kernel that held the
bound on the GPU did round to nearest even and did walk (ky, kx) in order."""
import numpy as np
import pytest
import torch

import test_gpu_conv_bf16_edges as edges
from _conv_bf16_ref import (TIE_CASES, bf16_half_away, bf16_round, bf16_truncate, operands, out_hw,
                            reference_backward, reference_forward)
from tensorium_amd._abi import ACT

LINEAR = ACT["LINEAR"]
ids = edges.ids
# each operand rounded wrongly; the last: nearest with ties away from zero for the operands
# that the kernels round in registers (pixels and deltas), the packed weights right
WRONG = {
    "truncation": dict(rnd_x=bf16_truncate, rnd_w=bf16_truncate, rnd_d=bf16_truncate),
    "half up in magnitude": dict(rnd_x=bf16_half_away, rnd_w=bf16_half_away,
                                 rnd_d=bf16_half_away),
    "half away, one operand": dict(rnd_d=bf16_half_away),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_rounding_vectors():
    v = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F7FFFFF, 0x80000000,
                  0x3F7F8000, 0x3F80FFFF], np.uint32).view(np.float32)
    assert bits(bf16_round(v)).tolist() == [0x3F800000, 0x3F820000, 0xBF800000, 0xBF820000,
                                            0x3F800000, 0x80000000, 0x3F800000, 0x3F810000]
    assert bits(bf16_truncate(v))[:2].tolist() == [0x3F800000, 0x3F810000]
    assert bits(bf16_half_away(v))[:4].tolist() == [0x3F810000, 0x3F820000, 0xBF810000, 0xBF820000]


@pytest.mark.parametrize("case", TIE_CASES, ids=ids)
def test_edge_data_composition(case):
    for name, a in operands(case, edges=True).items():
        u, n = bits(a).ravel(), a.size
        lo, odd, neg = u & 0xFFFF, (u >> 16) & 1 == 1, u >> 31 == 1
        tie = lo == 0x8000
        assert abs(tie.sum() / n - 0.25) < 1 / n + 1e-3, name
        if n >= 64:  # (not the bias vectors) exact ones and zeros; ties: parities and signs
            assert (lo == 0).sum() / n >= 0.25 + 0.05, name
            assert (lo == 0xFFFF).any() and (u == 0).any() and (u == 0x80000000).any(), name
            for p in (odd, ~odd):
                for s in (neg, ~neg):
                    assert (tie & p & s).any(), name
        mag = np.abs(a[a != 0])
        assert np.isfinite(a).all() and mag.min() >= 2.0 ** -20 and mag.max() <= 2.0
        assert np.isfinite(bf16_round(a)).all() and np.abs(bf16_round(a)).max() <= 2.0
    big = bits(operands(TIE_CASES[3], edges=True)["x"])
    assert ((big & 0x7FFFFFFF) == 0x3F7FFFFF).any()  # ... which rounds to 1.0


@pytest.mark.parametrize("case", edges.GEOMETRY + [edges.DW128] + TIE_CASES, ids=ids)
def test_references_match_autograd(case):
    """With the rounding taken out, the three float64 references are
    conv2d and its two gradients (every geometry the GPU tests use)."""
    C, H, W, filters, k, stride, pad, batch = case
    o = operands(case)
    same = lambda a: np.asarray(a, np.float64)  # noqa: E731
    x = torch.from_numpy(same(o["x"])).requires_grad_()
    w = torch.from_numpy(same(o["w"]).reshape(filters, C, k, k)).requires_grad_()
    y = torch.nn.functional.conv2d(x, w, torch.from_numpy(same(o["b"])), stride, pad)
    assert tuple(y.shape[2:]) == out_hw(H, W, k, stride, pad)
    y.backward(torch.from_numpy(same(o["d"])))
    ref, _ = reference_forward(torch, o["x"], o["w"], o["b"], k, stride, pad, LINEAR, rnd_x=same,
                               rnd_w=same)
    (rw, _), (rx, _) = reference_backward(torch, o["x"], o["w"], o["d"], k, stride, pad, o["wu0"],
                                          o["sd0"], rnd_x=same, rnd_w=same, rnd_d=same)
    assert np.abs(ref - y.detach().numpy()).max() < 1e-12
    assert np.abs(rw - o["wu0"] - w.grad.numpy().reshape(rw.shape)).max() < 1e-12
    assert np.abs(rx - o["sd0"] - x.grad.numpy().reshape(rx.shape)).max() < 1e-12


def results(case, **kw):
    k, stride, pad = case[4:7]
    o = operands(case, edges=True)
    fwd = {k_: v for k_, v in kw.items() if k_ != "rnd_d"}
    y = reference_forward(torch, o["x"], o["w"], o["b"], k, stride, pad, LINEAR, **fwd)
    dw, dx = reference_backward(torch, o["x"], o["w"], o["d"], k, stride, pad, o["wu0"], o["sd0"],
                                **kw)
    return dict(forward=y, dW=dw, dX=dx)


@pytest.mark.parametrize("case", TIE_CASES, ids=ids)
def test_bound_tells_the_rounding(case):
    """On the GPU tests' tie data, each wrong rounding of the operands breaks
    the bound somewhere in each of the three products, while the right
    rounding evaluated in fp32 (nearest, any order: at most (n + 1) 2^-24 S)
    stays within half of it."""
    right = results(case)
    fp32 = results(case, dtype=np.float32)
    for what, (ref, bound) in right.items():
        err = np.abs(fp32[what][0].astype(np.float64) - ref) / bound
        print(case, what, "fp32 evaluation: max err / bound", err.max())
        assert err.max() <= 0.5, what
    for name, kw in WRONG.items():
        wrong = results(case, **kw)
        for what, (ref, bound) in right.items():
            if name == "half away, one operand" and what == "forward":
                wrong[what] = results(case, rnd_x=bf16_half_away)[what]
            err = np.abs(wrong[what][0] - ref) / bound
            print(case, what, name, "max err / bound", err.max())
            assert err.max() > 1.0, f"{what}: {name} passes"


@pytest.mark.parametrize("case", [TIE_CASES[1], edges.GEOMETRY[7]], ids=ids)
def test_bound_tells_swapped_taps(case):
    """ky and kx exchanged (H != W, so nothing hides it) breaks every bound."""
    assert case[1] != case[2]
    right, wrong = results(case), results(case, swap=True)
    for what, (ref, bound) in right.items():
        err = np.abs(wrong[what][0] - ref) / bound
        print(case, what, "swapped taps: max err / bound", err.max())
        assert err.max() > 1.0, what


def test_cases_reach_their_branches():
    """The GPU case lists' comments against the planners' rules as
    conv_api.cpp states them: by shape the 64 x 64 tile everywhere, one
    slice but for the 13 x 13 tie case (two), the 128 x 128 dW tile for DW128
    alone."""
    for case in edges.GEOMETRY + [edges.DW128, edges.ACT_CASE] + TIE_CASES:
        C, H, W, filters, k, stride, pad, batch = case
        oh, ow = out_hw(H, W, k, stride, pad)
        assert oh > 0 and ow > 0
        for rows, cols in ((filters, batch * oh * ow), (C, batch * H * W)):
            assert not (rows >= 128 and -(-rows // 128) * -(-cols // 128) >= 512), case
        assert (filters >= 128 and C * k * k >= 128) == (case == edges.DW128), case
        # conv_bf16_dw_split: min(ceil(512 / tiles), steps / 8), at least 1
        bt = 128 if case == edges.DW128 else 64
        tiles, steps = -(-filters // bt) * -(-C * k * k // bt), -(-batch * oh * ow // 32)
        assert max(1, min(-(-512 // tiles), steps // 8)) == (2 if case == TIE_CASES[3] else 1), case
    assert sorted({c[5] for c in edges.GEOMETRY}) == [1, 2, 3, 4]
    assert sorted({c[4] for c in edges.GEOMETRY}) == [1, 2, 3, 5, 7]
    assert {out_hw(*c[1:3], *c[4:7]) for c in edges.GEOMETRY} >= {(1, 1), (1, 3)}
    assert max(c[0] for c in edges.GEOMETRY) > 128
    assert edges.DW128_SPLITS[-1] == -(-edges.DW128[7] * 49 // 32)
