"""The hazard table's completeness and its own safety (no GPU).

Every tns_hip_* entry point is classified exactly once — in the table
(tests/_hazard_cases.py), always-joins, never-joins or takes-no-context — so a
new entry point cannot be added without stating its hazards; and every
operand of every case, in every placement the device test uses, lies inside
the arena, clear of whatever it is not meant to meet.
"""
from types import SimpleNamespace

import pytest

import _hazard_cases as hz
from tensorium_amd import _abi


def test_every_entry_point_is_classified_exactly_once():
    names = [n for n in _abi.header_symbols() if n.startswith("tns_hip_")]
    classes = {"table": hz.TABLE_SYMBOLS, "always joins": hz.ALWAYS_JOINS,
               "never joins": hz.NEVER_JOINS, "no context": hz.NO_CONTEXT}
    where = {n: [k for k, s in classes.items() if n in s] for n in names}
    assert not {n: w for n, w in where.items() if len(w) != 1}, \
        "unclassified ([]) or doubly classified tns_hip_* entry points"
    stale = set().union(*classes.values()) - set(names)
    assert not stale, f"classified, but not in include/tns.h: {sorted(stale)}"


def test_the_table_covers_the_extent_shapes():
    """The shapes an extent can take are all there (the list of the issue
    this table answers): a case of each kind stays in the table."""
    ops = [(c, op) for c in hz.CASES for op in c.ops]
    assert any(op.first > 0 for _, op in ops)                       # element offsets
    assert any(op.first < 0 and op.last >= 0 for _, op in ops)      # negative increments
    assert any(op.i64 for _, op in ops)                             # int64 buffers
    assert any(op.null for _, op in ops)                            # optional operands
    assert any(op.role == "rw" for _, op in ops)                    # in-place / accumulate
    assert any(op.role == "side" for _, op in ops)                  # a second conv backward
    assert any(op.claim for _, op in ops)                           # pinned over-claims
    for c, op in ops:
        assert op.role in ("r", "w", "rw", "side"), (c.id, op.name)
        assert op.null or op.first <= op.last, (c.id, op.name)
        assert not op.claim or op.why, (c.id, op.name, "an over-claim says why")
        assert not op.i64 or (op.first % 2 == 0 and op.last % 2 == 1), (c.id, op.name)
    for r in hz.PENDING:
        assert r.r0 % 2 == 0 and r.r1 % 2 == 1, r.name


def _inside(lo, hi, region):
    return region[0] <= lo and hi < region[1]


def _meets(lo, hi, lo2, hi2):
    return lo <= hi2 and lo2 <= hi


@pytest.mark.parametrize("c", hz.CASES + hz.ALWAYS, ids=lambda c: c.id)
def test_every_placement_lies_inside_the_arena(c):
    names = [op.name for op in c.ops]
    assert len(set(names)) == len(names), c.id
    if c.args is not None:
        # the argument list matches the prototype (ctx first)
        p = SimpleNamespace(**{n: 4096 for n in names}, stream=None)
        assert len(c.args(p)) + 1 == len(_abi.PROTOTYPES[c.sym][1]), c.id
    # the quiet layout: inside the quiet region, operands apart
    quiet = hz.touched(c, hz.layout(c))
    for n, (lo, hi) in quiet.items():
        assert _inside(lo, hi, hz.QUIET), (c.id, n, lo, hi)
    spans = sorted(quiet.values())
    assert all(a[1] < b[0] for a, b in zip(spans, spans[1:])), (c.id, "operands overlap")
    if c in hz.ALWAYS:
        return
    for op, rng, placement in hz.trials(c):
        pos = hz.layout(c, op, rng, placement)
        t = hz.touched(c, pos)
        what = (c.id, op.name, rng.name, placement)
        for n, (lo, hi) in t.items():
            assert hz.MARGIN <= lo and hi < hz.ARENA - hz.MARGIN, (what, n, lo, hi)
            if n != op.name:
                assert (lo, hi) == quiet[n], (what, n)
        # the operand under test: against R exactly as the placement says ...
        f, l = pos[op.name] + op.extent[0], pos[op.name] + op.extent[1]
        shared = max(0, min(l, rng.r1) - max(f, rng.r0) + 1)
        assert shared == ((2 if op.i64 else 1) if placement in (2, 3) else 0), what
        gap = {1: rng.r0 - l, 2: 0, 3: 0, 4: f - rng.r1}[placement]
        assert gap in (0, 1), what
        if op.i64:
            assert pos[op.name] % 2 == 0, what
        # ... and clear of everything else: the other pending ranges, the
        # pending conv's other operands, the quiet region
        lo, hi = t[op.name]
        for other in hz.PENDING:
            assert other is rng or not _meets(lo, hi, other.r0, other.r1), (what, other.name)
        assert not _meets(lo, hi, hz.HOME[0], hz.HOME[1] - 1), what
        assert not _meets(lo, hi, hz.QUIET[0], hz.QUIET[1] - 1), what


def test_the_pending_conv_fits_its_home():
    assert hz.HOME_WEIGHTS + hz.P_W <= hz.HOME_OUTPUT
    assert hz.HOME_OUTPUT + hz.P_OUT <= hz.HOME_BIAS_UPDATES
    assert hz.HOME_BIAS_UPDATES + hz.PF <= hz.HOME[1]
    sizes = {"delta": hz.P_OUT, "input": hz.P_IN, "weight_updates": hz.P_W, "col": hz.P_COL}
    for r in hz.PENDING:
        assert r.r1 - r.r0 + 1 == sizes[r.name]
        assert hz.HOME[1] + hz.MARGIN <= r.r0 and r.r1 < hz.ARENA - hz.MARGIN


def test_the_rule():
    """expected_join restates check_ops: a write meets anything, a read only
    what the dW writes; read against read is the overlap the pipeline is for."""
    delta, wu = hz.PENDING[0], hz.PENDING[2]
    r, w, rw, side = (hz.Op("x", k, 0, 7) for k in ("r", "w", "rw", "side"))
    for pl in (2, 3):
        assert not hz.expected_join(r, delta, pl) and hz.expected_join(r, wu, pl)
        assert hz.expected_join(w, delta, pl) and hz.expected_join(rw, delta, pl)
        assert not hz.expected_join(side, wu, pl)
    for pl in (1, 4):
        assert not any(hz.expected_join(o, g, pl) for o in (r, w, rw, side) for g in (delta, wu))
