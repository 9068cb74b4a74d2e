"""Which calls join a pending dW of the pipelined conv backward, on the device.

A conv backward under TNS_OPT_BWD_OVERLAP = 2 leaves its dW product on the
side stream; tns_hip_pending_dw goes to 0 exactly when a later call joined it.
For every entry point of the hazard table (tests/_hazard_cases.py), every
operand and every range of the pending dW (delta and input, which it reads;
weight_updates and the caller's col workspace, which it writes) the operand is
placed four ways against the range — ending just below it, sharing its first
element, sharing its last, starting just above — with every other operand far
away, and the join is held against the rule of check_ops (csrc/tns_ctx.hpp):
a call joins iff it writes a range the dW reads or writes, or reads one the dW
writes.  Exact booleans: no race, no timing.  Everything lives in one arena
tensor, so adjacency is exact to the element, and tests/test_hazards.py holds
every placement inside it.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import _hazard_cases as hz

pytestmark = pytest.mark.gpu


class Env:
    def __init__(self, hip, T):
        self.hip, self.T, self.lib = hip, T, hip.lib
        i = np.arange(hz.ARENA, dtype=np.int64)
        host = (0.25 + 0.5 * ((i * 37) % 101) / 101.0).astype(np.float32)  # finite, in (0, 1)
        self.pristine = T.from_numpy(host).cuda()
        self.arena = T.empty(hz.ARENA, dtype=T.float32, device="cuda")
        self.base = self.arena.data_ptr()
        assert self.base % 16 == 0
        self.stream = hip.stream   # (taken now: the property joins)

    def view(self, at, n):
        return self.arena[at:at + n]

    def reset(self, c, pos):
        """All memory finite; the int64 / list operands a kernel reads zeroed."""
        self.arena.copy_(self.pristine)
        for op in c.ops:
            if op.zero and not op.null:
                self.arena[pos[op.name] + op.first:pos[op.name] + op.last + 1] = 0.0
        self.T.cuda.synchronize()

    def queue_dw(self):
        """The pending dW: its delta, input, weight_updates and col workspace
        at the table's positions; precondition pendingDw() == 1."""
        at = {r.name: r.r0 for r in hz.PENDING}
        v = self.view
        self.hip.finish()   # (nothing left over from a trial that failed half-way)
        self.hip.convBackward(hz.PB, hz.PC, hz.PH, hz.PH, v(at["input"], hz.P_IN),
                              v(hz.HOME_WEIGHTS, hz.P_W), hz.PF, hz.PK, 1, 1, 1, hz.LEAKY,
                              v(hz.HOME_OUTPUT, hz.P_OUT), v(at["delta"], hz.P_OUT),
                              v(hz.HOME_BIAS_UPDATES, hz.PF), v(at["weight_updates"], hz.P_W),
                              v(at["col"], hz.P_COL), None)
        assert self.hip.pendingDw() == 1, "precondition: the conv backward left its dW pending"

    def call(self, c, pos):
        p = hz.pointers(c, pos, self.base, stream=self.stream)
        rc = getattr(self.lib, c.sym)(self.hip.ctx, *c.args(p))
        return rc

    def settle(self):
        self.hip.finish()
        assert self.hip.pendingDw() == 0


@pytest.fixture(scope="module")
def env(hip, torch_cuda):
    """The arena, and the options that make the dW pend and fill the caller's
    col workspace (no residue form, no implicit-im2col tile: im2col + sdot);
    every option back at its default afterwards."""
    e = Env(hip, torch_cuda)
    try:
        hip.setBwdOverlap(2)
        hip.setDwRes(-2)
        hip.setDwTile(-2)
        hip.finish()
        yield e
    finally:
        hip.setDwRes(-1)
        hip.setDwTile(-1)
        hip.setBwdOverlap(True)
        hip.finish()


def _status(env, rc, what):
    if rc != 0:
        msg = env.lib.tns_last_error().decode(errors="replace")
        env.lib.tns_clear_error()
        env.settle()
        pytest.fail(f"{what}: status {rc}: {msg}")


@pytest.mark.parametrize("c", hz.CASES, ids=lambda c: c.id)
def test_join_at_the_edges_of_every_pending_range(env, c):
    wrong = []
    for op, rng, placement in hz.trials(c):
        pos = hz.layout(c, op, rng, placement)
        env.reset(c, pos)
        env.queue_dw()
        rc = env.call(c, pos)
        after = env.hip.pendingDw()
        _status(env, rc, (c.sym, c.id, op.name, rng.name, placement))
        assert after in (c.adds_pending, 1 + c.adds_pending), after
        joined, expect = after == c.adds_pending, hz.expected_join(op, rng, placement)
        env.settle()
        if joined != expect:
            wrong.append(f"{c.sym} [{c.id}] operand {op.name} ({op.role}) against the pending "
                         f"{rng.name} ({'written' if rng.written else 'read'}), placement "
                         f"{placement}: expected {'a join' if expect else 'no join'}, observed "
                         f"{'a join' if joined else 'no join'}"
                         f" ({'missed join' if expect else 'needless join'})")
    assert not wrong, "\n" + "\n".join(wrong)


@pytest.mark.parametrize("c", hz.CASES, ids=lambda c: c.id)
def test_no_join_with_every_operand_far_away(env, c):
    """The quiet layout joins nothing: what the edge placements are measured
    against."""
    pos = hz.layout(c)
    env.reset(c, pos)
    env.queue_dw()
    rc = env.call(c, pos)
    after = env.hip.pendingDw()
    _status(env, rc, (c.sym, c.id))
    env.settle()
    assert after == 1 + c.adds_pending, (c.sym, c.id, "joined with nothing near a pending range")


@pytest.mark.parametrize("c", hz.ALWAYS, ids=lambda c: c.id)
def test_entry_points_that_always_join(env, c):
    """check_ctx's default: operands far from everything, pending goes to 0."""
    pos = hz.layout(c)
    env.reset(c, pos)
    if c.sym == "tns_hip_mlp_train_step":
        need = env.hip.mlpBufferFloats(list(hz.MLP_WIDTHS), 0, hz.MLP_BATCH)
        assert 0 < need <= hz.MLP_BUF_BOUND, need
    env.queue_dw()
    if c.sym in ("tns_hip_malloc", "tns_hip_free"):
        # malloc joins; the dW queued again, free joins
        got = C.c_void_p()
        rc = env.lib.tns_hip_malloc(env.hip.ctx, 16, C.byref(got))
        after = env.hip.pendingDw()
        if c.sym == "tns_hip_free":
            assert rc == 0 and after == 0
            env.queue_dw()
        rc2 = env.lib.tns_hip_free(env.hip.ctx, got) if rc == 0 else 0
        if c.sym == "tns_hip_free":
            rc, after = rc2, env.hip.pendingDw()
        _status(env, rc or rc2, c.sym)
    elif c.sym == "tns_hip_get_stream":
        assert int(env.lib.tns_hip_get_stream(env.hip.ctx) or 0) == env.stream
        after = env.hip.pendingDw()
    else:
        rc = env.call(c, pos)
        after = env.hip.pendingDw()
        _status(env, rc, c.sym)
    env.settle()
    assert after == 0, (c.sym, "left the dW pending")


def test_the_getters_never_join(env):
    c = SimpleNamespace(ops=())
    env.reset(c, {})
    env.queue_dw()
    try:
        assert env.lib.tns_hip_pending_dw(env.hip.ctx) == 1
        env.lib.tns_hip_op_ms(env.hip.ctx, 0)
        assert env.hip.pendingDw() == 1, "tns_hip_op_ms joined"
        assert env.hip.pendingDw() == 1, "tns_hip_pending_dw joined"
    finally:
        env.settle()
