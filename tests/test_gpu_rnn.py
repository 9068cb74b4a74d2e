"""rnnStateForward / rnnDeltaBackward, bit for bit (uint32 views), against

* tests/_rnn_oracle.py's per-element restatement (state_forward /
  delta_backward), and
* the literal sequence of existing TNNHip calls the reference's CPU path maps
  to (forwardBias, ActivateArray, fill or copy, addvv, addvv; clamp,
  DeriveArray, copy, clamp, DeriveArray), run on the device,

at N in {1, 3, 15, 16, 1027} and, past one block with a bias row that is no
multiple of the 4-element item, 1040, with H dividing N; every operand 16-byte
aligned (the float4 path) and one float off (the scalar path); bias given and
null; state_prev null, a slice of its own and state_next itself; delta2 null
and given; LOGISTIC, TANH, LEAKY, RELU and LINEAR.  Guard floats after every
operand stay unchanged.  Inputs hold +-0 (a = b = -0 at element 0: the sum is
+0), denormals and +-30; deltas lie in [-3, 3] with +-0 and a NaN, which stays
a NaN (NaN positions are compared, not their payloads).  Every TNS_ERR_ARG /
TNS_ERR_UNSUPPORTED case leaves every operand untouched."""
import numpy as np
import pytest

from tensorium_amd._abi import ACT, TnsError

import _rnn_oracle as ro

pytestmark = pytest.mark.gpu

CASES = [(1, 1), (3, 1), (3, 3), (15, 5), (15, 1), (16, 8), (16, 1), (1027, 1), (1027, 13),
         (1040, 5), (1040, 8)]
ACTS = ["LOGISTIC", "TANH", "LEAKY", "RELU", "LINEAR"]
GUARD = 8
MARK = np.float32(-77.25)
SPECIAL = np.array([-0.0, 0.0, 1e-40, -1e-40, 1.4e-45, 30.0, -30.0], np.float32)
u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731


class Arena:
    """Operands in one device buffer, each at a 16-byte boundary plus `shift`
    floats, with GUARD marked floats after each."""

    def __init__(self, T, sizes, shift):
        self.sizes, self.off, at = sizes, {}, 0
        for k, n in sizes.items():
            self.off[k] = at + shift
            at += (n + GUARD + shift + 3) // 4 * 4 + 4
        self.host = np.full(at, MARK, np.float32)
        self.T = T

    def put(self, k, a):
        self.host[self.off[k]:self.off[k] + self.sizes[k]] = a

    def upload(self):
        self.dev = self.T.from_numpy(self.host.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        return self

    def p(self, k):
        return self.dev.data_ptr() + 4 * self.off[k]

    def get(self):
        h = self.dev.cpu().numpy()
        out = {k: h[self.off[k]:self.off[k] + n].copy() for k, n in self.sizes.items()}
        keep = np.ones(h.size, bool)
        for k, n in self.sizes.items():
            keep[self.off[k]:self.off[k] + n] = False
        assert (h[keep] == MARK).all(), "a guard float was written"
        return out

    def untouched(self):
        return np.array_equal(u32(self.dev.cpu().numpy()), u32(self.host))


def same(got, want, keys, what):
    bad = []
    for k in keys:
        g, w = got[k], np.ascontiguousarray(want[k], np.float32)
        nan = np.isnan(w)
        if not (np.array_equal(nan, np.isnan(g)) and np.array_equal(u32(g)[~nan], u32(w)[~nan])):
            bad.append((what, k, int((u32(g) != u32(w)).sum())))
    assert not bad, bad


# ---- forward ---------------------------------------------------------------------------

def fwd_operands(N, H, seed):
    rng = np.random.default_rng(seed)
    r = lambda lo, hi, n=N: rng.uniform(lo, hi, n).astype(np.float32)  # noqa: E731
    d = dict(a=r(-3, 3), b=r(-3, 3), prev=r(-2, 2), ab=r(-0.5, 0.5, H), bb=r(-0.5, 0.5, H))
    m = min(N, SPECIAL.size)
    d["a"][:m] = SPECIAL[:m]
    d["b"][:m] = SPECIAL[:m][::-1] if m > 1 else SPECIAL[:1]
    d["b"][0] = -0.0          # a[0] = b[0] = -0
    if N > 1:
        d["prev"][1] = -0.0
    return d


FWD = ("a", "b", "ab", "bb", "prev", "next")


def fwd_arena(T, d, N, H, shift, mode):
    a = Arena(T, dict(a=N, b=N, ab=H, bb=H, prev=N, next=N), shift)
    for k in ("a", "b", "ab", "bb", "prev"):
        a.put(k, d[k])
    if mode == "same":
        a.put("next", d["prev"])
    return a.upload()


def run_state_forward(hip, T, d, N, H, shift, bias, mode, acts):
    a = fwd_arena(T, d, N, H, shift, mode)
    prev = {"null": None, "own": a.p("prev"), "same": a.p("next")}[mode]
    hip.rnnStateForward(N, H, a.p("a"), a.p("ab") if bias else None, acts[0], a.p("b"),
                        a.p("bb") if bias else None, acts[1], prev, a.p("next"))
    hip.finish()
    return a.get()


def literal_state_forward(hip, T, d, N, H, bias, mode, acts):
    a = fwd_arena(T, d, N, H, 0, mode)
    p = a.p
    for x, b, act in (("a", "ab", acts[0]), ("b", "bb", acts[1])):
        if bias:
            hip.forwardBias(N, p(x), 0, H, p(b), 1, N // H)
        hip.ActivateArray(N, p(x), 0, act)
    if mode == "null":
        hip.fill(N, p("next"), 0, 0.0, 1)
    elif mode == "own":
        hip.copy(N, p("prev"), 0, 1, p("next"), 0, 1)
    hip.addvv(N, p("next"), 0, 1, p("a"), 0, 1, p("next"), 0, 1)
    hip.addvv(N, p("next"), 0, 1, p("b"), 0, 1, p("next"), 0, 1)
    hip.finish()
    return a.get()


@pytest.mark.parametrize("act", range(len(ACTS)))
@pytest.mark.parametrize("N, H", CASES)
def test_state_forward(hip, torch_cuda, ora, N, H, act):
    acts = (ACT[ACTS[act]], ACT[ACTS[(act + 1) % len(ACTS)]])
    d = fwd_operands(N, H, 1000 * act + N + H)
    for bias in (True, False):
        for mode in ("null", "own", "same"):
            wa, wb, ws = ro.state_forward(ora, d["a"], d["ab"] if bias else None, acts[0], d["b"],
                                          d["bb"] if bias else None, acts[1],
                                          None if mode == "null" else d["prev"], H)
            assert all(np.isfinite(v).all() for v in (wa, wb, ws))
            want = dict(d, a=wa, b=wb, next=ws)
            if not bias and mode == "null" and {ACTS[act], ACTS[(act + 1) % 5]} <= {
                    "LEAKY", "RELU", "LINEAR"}:
                assert u32(wa)[0] == u32(wb)[0] == 0x80000000 and u32(ws)[0] == 0  # (0 + -0) + -0
            for shift in (0, 1):
                got = run_state_forward(hip, torch_cuda, d, N, H, shift, bias, mode, acts)
                same(got, want, FWD, f"oracle bias={bias} prev={mode} shift={shift}")
            lit = literal_state_forward(hip, torch_cuda, d, N, H, bias, mode, acts)
            same(lit, want, FWD, f"literal bias={bias} prev={mode}")


# ---- backward --------------------------------------------------------------------------

def bwd_operands(ora, N, seed, acts):
    rng = np.random.default_rng(seed)
    r = lambda lo, hi: rng.uniform(lo, hi, N).astype(np.float32)  # noqa: E731
    d = dict(delta=r(-3, 3), out=ora.activate(r(-3, 3), acts[0]),
             out2=ora.activate(r(-3, 3), acts[1]))
    d["delta"][0] = -0.0
    if N >= 3:
        d["delta"][1] = np.nan
        d["delta"][2] = 0.0
    if N >= 15:
        d["delta"][3:7] = [1.0, -1.0, 1.0000001, -2.5]
        d["out"][7:9] = [0.0, -0.0]
    return d


BWD = ("delta", "out", "delta2", "out2")


def bwd_arena(T, d, N, shift):
    a = Arena(T, dict(delta=N, out=N, delta2=N, out2=N), shift)
    for k in ("delta", "out", "out2"):
        a.put(k, d[k])
    return a.upload()


def run_delta_backward(hip, T, d, N, shift, two, acts):
    a = bwd_arena(T, d, N, shift)
    if two:
        hip.rnnDeltaBackward(N, a.p("delta"), a.p("out"), acts[0], a.p("delta2"), a.p("out2"),
                             acts[1])
    else:
        hip.rnnDeltaBackward(N, a.p("delta"), a.p("out"), acts[0])
    hip.finish()
    return a.get()


def literal_delta_backward(hip, T, d, N, two, acts):
    a = bwd_arena(T, d, N, 0)
    p = a.p
    hip.clamp(N, 1.0, p("delta"), p("delta"))
    hip.DeriveArray(N, p("out"), 0, acts[0], p("delta"))
    if two:
        hip.copy(N, p("delta"), 0, 1, p("delta2"), 0, 1)
        hip.clamp(N, 1.0, p("delta2"), p("delta2"))
        hip.DeriveArray(N, p("out2"), 0, acts[1], p("delta2"))
    hip.finish()
    return a.get()


@pytest.mark.parametrize("act", range(len(ACTS)))
@pytest.mark.parametrize("N", sorted({n for n, _ in CASES}))
def test_delta_backward(hip, torch_cuda, ora, N, act):
    acts = (ACT[ACTS[act]], ACT[ACTS[(act + 2) % len(ACTS)]])
    d = bwd_operands(ora, N, 2000 * act + N, acts)
    mark = np.full(N, MARK, np.float32)
    for two in (False, True):
        w1, w2 = ro.delta_backward(ora, d["delta"], d["out"], acts[0],
                                   d["out2"] if two else None, acts[1])
        nan = np.isnan(d["delta"])
        assert np.array_equal(np.isnan(w1), nan) and np.abs(w1[~nan]).max(initial=0) <= 1.0
        if two:
            assert np.array_equal(np.isnan(w2), nan)
        want = dict(d, delta=w1, delta2=w2 if two else mark)
        for shift in (0, 1):
            got = run_delta_backward(hip, torch_cuda, d, N, shift, two, acts)
            same(got, want, BWD, f"oracle delta2={two} shift={shift}")
        same(literal_delta_backward(hip, torch_cuda, d, N, two, acts), want, BWD,
             f"literal delta2={two}")


def test_the_clamp_is_exercised(ora):
    """(no GPU work) both clamps change something: |delta| > 1 going in."""
    acts = (ACT["LINEAR"], ACT["LEAKY"])
    d = bwd_operands(ora, 1027, 5, acts)
    w1, _ = ro.delta_backward(ora, d["delta"], d["out"], acts[0])
    assert (np.abs(d["delta"]) > 1).sum() > 100 and (np.abs(w1) == 1.0).sum() > 100


# ---- arguments -------------------------------------------------------------------------

def test_bad_arguments_leave_every_operand_untouched(hip, torch_cuda, ora):
    N, H = 10, 5
    d = fwd_operands(N, H, 7)
    e = bwd_operands(ora, N, 8, (ACT["TANH"], ACT["LEAKY"]))
    LEAKY, ELU = ACT["LEAKY"], ACT["ELU"]

    def fwd(status, **kw):
        a = fwd_arena(torch_cuda, d, N, H, 0, "own")
        q = dict(N=N, H=H, a=a.p("a"), ab=a.p("ab"), ia=LEAKY, b=a.p("b"), bb=a.p("bb"), sa=LEAKY,
                 prev=a.p("prev"), next=a.p("next"))
        q.update({k: (v(q) if callable(v) else v) for k, v in kw.items()})
        with pytest.raises(TnsError, match=f"tns status {status}"):
            hip.rnnStateForward(q["N"], q["H"], q["a"], q["ab"], q["ia"], q["b"], q["bb"], q["sa"],
                                q["prev"], q["next"])
        hip.finish()
        assert a.untouched(), kw

    def bwd(status, **kw):
        a = bwd_arena(torch_cuda, e, N, 0)
        q = dict(N=N, delta=a.p("delta"), out=a.p("out"), act=LEAKY, delta2=a.p("delta2"),
                 out2=a.p("out2"), act2=LEAKY)
        q.update({k: (v(q) if callable(v) else v) for k, v in kw.items()})
        with pytest.raises(TnsError, match=f"tns status {status}"):
            hip.rnnDeltaBackward(q["N"], q["delta"], q["out"], q["act"], q["delta2"], q["out2"],
                                 q["act2"])
        hip.finish()
        assert a.untouched(), kw

    fwd(1, N=-1)
    fwd(1, H=0)
    fwd(1, H=-3)
    fwd(1, a=None)
    fwd(1, b=None)
    fwd(1, next=None)
    fwd(1, b=lambda q: q["a"])                        # two outputs
    fwd(1, next=lambda q: q["a"] + 4 * (N - 1))       # partly
    fwd(1, next=lambda q: q["prev"] + 4)              # state_prev, but not the same slice
    fwd(1, a=lambda q: q["prev"])                     # an output on an input
    fwd(1, b=lambda q: q["bb"] - 4 * (N - 1))         # an output reaching a bias
    fwd(1, next=lambda q: q["ab"])
    fwd(4, ia=ELU)
    fwd(4, sa=ACT["LOGGY"])
    fwd(4, ia=99)
    bwd(1, N=-1)
    bwd(1, delta=None)
    bwd(1, out=None)
    bwd(1, out2=None)                                 # delta2 given without its out2
    bwd(1, delta2=lambda q: q["delta"])
    bwd(1, delta2=lambda q: q["out"] + 4)
    bwd(1, delta=lambda q: q["out2"])
    bwd(1, delta=lambda q: q["out"] - 4 * (N - 1))
    bwd(4, act=ELU)
    bwd(4, act2=ELU)
    # N == 0 does nothing, whatever the pointers; inputs may meet one another;
    # act2 / out2 are not looked at without delta2
    a = bwd_arena(torch_cuda, e, N, 0)
    hip.rnnStateForward(0, 1, None, None, LEAKY, None, None, LEAKY, None, None)
    hip.rnnDeltaBackward(0, None, None, LEAKY)
    hip.finish()
    assert a.untouched()
    hip.rnnDeltaBackward(N, a.p("delta"), a.p("out"), LEAKY, None, None, ELU)
    hip.rnnDeltaBackward(N, a.p("delta"), a.p("out"), LEAKY, a.p("delta2"), a.p("out"), LEAKY)
    f = fwd_arena(torch_cuda, d, N, H, 0, "own")
    hip.rnnStateForward(N, H, f.p("a"), f.p("ab"), LEAKY, f.p("b"), f.p("ab"), LEAKY, f.p("prev"),
                        f.p("next"))
    hip.finish()
    f.get()
    a.get()
