"""lstmGatesForward / lstmGatesBackward, bit for bit (uint32 views), against

* tests/_lstm_oracle.py's per-element restatement (gates_forward /
  gates_backward), and
* the literal sequence of existing TNNHip calls TLSTMLayer.forwardGPU /
  backwardGPU make (nlstmlayer.pas:933-973, 1046-1255), with the clamp that
  opens each sub-layer's backward, run on the device,

at sizes around the 4-element item and the 256-thread block, with every
operand 16-byte aligned (the float4 path) and one float off (the scalar path),
and guard floats after every operand unchanged.  Pre-activations are U[-6, 6]
plus a handful of +-0.0, denormals and +-30, which stay finite through the
reference's tanh form (checked on the oracle's results).  The TNS_ERR_ARG cases
leave every output untouched."""
import numpy as np
import pytest

from tensorium_amd._abi import ACT, TnsError

import _lstm_oracle as lo

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023]
GUARD = 8
MARK = np.float32(-77.25)
SPECIAL = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 30.0, -30.0], np.float32)
u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731


def operands(N, seed):
    """The 8 pre-activation slices and the state / gradient operands."""
    rng = np.random.default_rng(seed)
    r = lambda lo_, hi: rng.uniform(lo_, hi, N).astype(np.float32)  # noqa: E731
    d = {k: r(-3, 3) for k in ("wf", "wi", "wg", "wo", "uf", "ui", "ug", "uo")}
    for k in ("wf", "wi", "wg", "wo"):      # the sums: U[-6, 6] and the specials
        m = min(N, SPECIAL.size)
        if m:
            at = rng.permutation(N)[:m]
            d[k][at] = SPECIAL[:m]
            d["u" + k[1]][at] = 0.0
    d.update(c=r(-2, 2), cell=r(-2, 2), cprev=r(-2, 2), delta=r(-3, 3), dc=r(-2, 2))
    return d


class Arena:
    """Operands in one device buffer, each at a 16-byte boundary plus `shift`
    floats, with GUARD marked floats after each."""

    def __init__(self, T, names, N, shift):
        self.N, self.names = N, names
        self.stride = (N + GUARD + shift + 3) // 4 * 4 + 4
        self.off = {k: i * self.stride + shift for i, k in enumerate(names)}
        self.host = np.full(self.stride * len(names), MARK, np.float32)
        self.T = T

    def put(self, k, a):
        self.host[self.off[k]:self.off[k] + self.N] = a

    def upload(self):
        self.dev = self.T.from_numpy(self.host.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        return self

    def p(self, k):
        return self.dev.data_ptr() + 4 * self.off[k]

    def get(self):
        h = self.dev.cpu().numpy()
        out = {k: h[self.off[k]:self.off[k] + self.N].copy() for k in self.names}
        keep = np.ones(h.size, bool)
        for k in self.names:
            keep[self.off[k]:self.off[k] + self.N] = False
        assert (h[keep] == MARK).all(), "a guard float was written"
        return out


PRE = ("wf", "wi", "wg", "wo", "uf", "ui", "ug", "uo")
FWD = PRE + ("c", "h", "cell_out", "out")
BWD = PRE + ("cell", "cprev", "delta", "dc", "dwf", "dwi", "dwg", "dwo", "duf", "dui", "dug",
             "duo")
TMP = ("_f", "_i", "_g", "_o", "t1", "t2", "t3")


def run_forward(hip, T, d, N, shift):
    a = Arena(T, FWD, N, shift)
    for k in PRE + ("c",):
        a.put(k, d[k])
    a.upload()
    hip.lstmGatesForward(N, [a.p(k) for k in PRE[:4]], [a.p(k) for k in PRE[4:]], a.p("c"),
                         a.p("h"), a.p("cell_out"), a.p("out"))
    hip.finish()
    return a.get()


def run_backward(hip, T, d, N, shift, with_u=True):
    a = Arena(T, BWD, N, shift)
    for k in PRE + ("cell", "cprev", "delta", "dc"):
        a.put(k, d[k])
    a.upload()
    hip.lstmGatesBackward(N, [a.p(k) for k in PRE[:4]], [a.p(k) for k in PRE[4:]], a.p("cell"),
                          a.p("cprev"), a.p("delta"), a.p("dc"),
                          [a.p(k) for k in ("dwf", "dwi", "dwg", "dwo")],
                          [a.p(k) for k in ("duf", "dui", "dug", "duo")] if with_u else None)
    hip.finish()
    return a.get()


def literal_gates(hip, a, N):
    for g in "figo":
        hip.addvv(N, a.p("w" + g), 0, 1, a.p("u" + g), 0, 1, a.p("_" + g), 0, 1)
    hip.ActivateArray(N, a.p("_f"), 0, ACT["LOGISTIC"])
    hip.ActivateArray(N, a.p("_i"), 0, ACT["LOGISTIC"])
    hip.ActivateArray(N, a.p("_o"), 0, ACT["LOGISTIC"])
    hip.ActivateArray(N, a.p("_g"), 0, ACT["TANH"])


def literal_forward(hip, T, d, N):
    a = Arena(T, FWD + TMP, N, 0)
    for k in PRE + ("c",):
        a.put(k, d[k])
    a.upload()
    literal_gates(hip, a, N)
    hip.mulvv(N, a.p("_i"), 0, 1, a.p("_g"), 0, 1, a.p("t1"), 0, 1)
    hip.fmavv(N, a.p("c"), 0, 1, a.p("_f"), 0, 1, a.p("t1"), 0, 1, a.p("c"), 0, 1)
    hip.copy(N, a.p("c"), 0, 1, a.p("h"), 0, 1)
    hip.ActivateArray(N, a.p("h"), 0, ACT["TANH"])
    hip.mulvv(N, a.p("_o"), 0, 1, a.p("h"), 0, 1, a.p("h"), 0, 1)
    hip.copy(N, a.p("c"), 0, 1, a.p("cell_out"), 0, 1)
    hip.copy(N, a.p("h"), 0, 1, a.p("out"), 0, 1)
    hip.finish()
    return a.get()


def literal_backward(hip, T, d, N):
    a = Arena(T, BWD + TMP, N, 0)
    for k in PRE + ("cell", "cprev", "delta", "dc"):
        a.put(k, d[k])
    a.upload()
    p = a.p
    literal_gates(hip, a, N)
    hip.copy(N, p("delta"), 0, 1, p("t3"), 0, 1)
    hip.copy(N, p("cell"), 0, 1, p("t1"), 0, 1)
    hip.ActivateArray(N, p("t1"), 0, ACT["TANH"])
    hip.mulvv(N, p("t3"), 0, 1, p("_o"), 0, 1, p("t2"), 0, 1)
    hip.DeriveArray(N, p("t1"), 0, ACT["TANH"], p("t2"))
    hip.addvv(N, p("dc"), 0, 1, p("t2"), 0, 1, p("t2"), 0, 1)
    hip.copy(N, p("cell"), 0, 1, p("t1"), 0, 1)
    hip.ActivateArray(N, p("t1"), 0, ACT["TANH"])
    hip.mulvv(N, p("t3"), 0, 1, p("t1"), 0, 1, p("t1"), 0, 1)
    hip.DeriveArray(N, p("_o"), 0, ACT["LOGISTIC"], p("t1"))
    for g, other, act in (("o", None, None), ("g", "_i", "TANH"), ("i", "_g", "LOGISTIC"),
                          ("f", "cprev", "LOGISTIC")):
        if other is not None:
            hip.mulvv(N, p("t2"), 0, 1, p(other), 0, 1, p("t1"), 0, 1)
            hip.DeriveArray(N, p("_" + g), 0, ACT[act], p("t1"))
        for side in "wu":   # temp.copyTo(x.delta), then the sub-layer's clamp(delta, 1)
            hip.copy(N, p("t1"), 0, 1, p("d" + side + g), 0, 1)
            hip.clamp(N, 1.0, p("d" + side + g), p("d" + side + g))
    hip.mulvv(N, p("t2"), 0, 1, p("_f"), 0, 1, p("t1"), 0, 1)
    hip.copy(N, p("t1"), 0, 1, p("dc"), 0, 1)
    hip.finish()
    return a.get()


def same(got, want, keys, what):
    bad = [(what, k, int((u32(got[k]) != u32(want[k])).sum())) for k in keys
           if not np.array_equal(u32(got[k]), u32(want[k]))]
    assert not bad, bad


@pytest.mark.parametrize("N", SIZES)
def test_gates_forward(hip, torch_cuda, ora, N):
    d = operands(N, 100 + N)
    w, u = [d[k] for k in PRE[:4]], [d[k] for k in PRE[4:]]
    c, h = (lo.gates_forward(ora, w, u, d["c"]) if N else
            (np.zeros(0, np.float32), np.zeros(0, np.float32)))
    assert np.isfinite(c).all() and np.isfinite(h).all()
    want = dict(d, c=c, h=h, cell_out=c, out=h)
    keys = FWD if N else ()
    for shift in (0, 1):
        same(run_forward(hip, torch_cuda, d, N, shift), want, keys, f"oracle shift {shift}")
    if N:
        same(run_forward(hip, torch_cuda, d, N, 0), literal_forward(hip, torch_cuda, d, N), FWD,
             "literal")


@pytest.mark.parametrize("N", SIZES)
def test_gates_backward(hip, torch_cuda, ora, N):
    d = operands(N, 200 + N)
    if N:
        w, u = [d[k] for k in PRE[:4]], [d[k] for k in PRE[4:]]
        (df, di, dg, do), dc = lo.gates_backward(ora, w, u, d["cell"], d["cprev"], d["delta"],
                                                 d["dc"])
        for a in (df, di, dg, do, dc):
            assert np.isfinite(a).all()
        assert max(np.abs(a).max() for a in (df, di, dg, do)) <= 1.0
        want = dict(d, dc=dc, dwf=df, dwi=di, dwg=dg, dwo=do, duf=df, dui=di, dug=dg, duo=do)
    for shift in (0, 1):
        got = run_backward(hip, torch_cuda, d, N, shift)
        if N:
            same(got, want, BWD, f"oracle shift {shift}")
    if N:
        same(run_backward(hip, torch_cuda, d, N, 0), literal_backward(hip, torch_cuda, d, N), BWD,
             "literal")
        got = run_backward(hip, torch_cuda, d, N, 1, with_u=False)   # no u-side slices given
        same(got, want, BWD[:16], "no du")
        assert all((got[k] == MARK).all() for k in ("duf", "dui", "dug", "duo"))


def test_the_clamp_is_exercised(ora):
    """(no GPU work) the operands above do produce gate deltas beyond +-1."""
    d = operands(1023, 200 + 1023)
    w, u = [d[k] for k in PRE[:4]], [d[k] for k in PRE[4:]]
    (df, di, dg, do), _ = lo.gates_backward(ora, w, u, d["cell"], d["cprev"], d["delta"], d["dc"])
    assert any((np.abs(a) == 1.0).any() for a in (df, di, dg, do))


def test_bad_arguments_leave_the_outputs_untouched(hip, torch_cuda):
    N = 9
    d = operands(N, 7)

    def fwd(change):
        a = Arena(torch_cuda, FWD, N, 0)
        for k in PRE + ("c",):
            a.put(k, d[k])
        a.upload()
        p = {k: a.p(k) for k in FWD}
        n = change(p) or N
        with pytest.raises(TnsError):
            hip.lstmGatesForward(n, [p[k] for k in PRE[:4]], [p[k] for k in PRE[4:]], p["c"],
                                 p["h"], p["cell_out"], p["out"])
        hip.finish()
        assert np.array_equal(u32(a.dev.cpu().numpy()), u32(a.host))

    def bwd(change):
        a = Arena(torch_cuda, BWD, N, 0)
        for k in PRE + ("cell", "cprev", "delta", "dc"):
            a.put(k, d[k])
        a.upload()
        p = {k: a.p(k) for k in BWD}
        n = change(p) or N
        with pytest.raises(TnsError):
            hip.lstmGatesBackward(n, [p[k] for k in PRE[:4]], [p[k] for k in PRE[4:]], p["cell"],
                                  p["cprev"], p["delta"], p["dc"],
                                  [p[k] for k in ("dwf", "dwi", "dwg", "dwo")],
                                  [p[k] for k in ("duf", "dui", "dug", "duo")])
        hip.finish()
        assert np.array_equal(u32(a.dev.cpu().numpy()), u32(a.host))

    def setp(k, v):
        def change(p):
            p[k] = v(p) if callable(v) else v
        return change

    fwd(lambda p: -1)
    fwd(setp("wg", None))
    fwd(setp("h", None))
    fwd(setp("h", lambda p: p["c"]))                 # two outputs
    fwd(setp("cell_out", lambda p: p["out"] + 4))    # partly
    fwd(setp("out", lambda p: p["uo"]))              # an output on an input
    fwd(setp("c", lambda p: p["wf"] + 4 * (N - 1)))
    bwd(lambda p: -1)
    bwd(setp("cprev", None))
    bwd(setp("dwi", None))
    bwd(setp("dc", lambda p: p["delta"]))
    bwd(setp("dwf", lambda p: p["dwo"]))
    bwd(setp("duf", lambda p: p["dwf"]))             # the u side must be a separate slice
    bwd(setp("dug", lambda p: p["cell"] - 4))
    # inputs may meet one another; N == 0 does nothing, whatever the pointers
    a = Arena(torch_cuda, BWD, N, 0).upload()
    hip.lstmGatesBackward(0, [None] * 4, [None] * 4, None, None, None, None, [None] * 4)
    hip.lstmGatesForward(0, [None] * 4, [None] * 4, None, None, None, None)
    hip.lstmGatesBackward(N, [a.p("wf")] * 4, [a.p("wf")] * 4, a.p("cell"), a.p("cell"),
                          a.p("cell"), a.p("dc"), [a.p(k) for k in ("dwf", "dwi", "dwg", "dwo")])
    hip.finish()
