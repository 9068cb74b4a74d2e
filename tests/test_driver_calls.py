"""The backend calls the darknet drivers make, pinned without a GPU.

tests/_driver_trace.py drives HipDarknet and HipDarknetTrain on CPU tensors
against a recording stand-in for TNNHip; tests/golden/driver_calls.json holds,
per case and phase (forward, backward, update), the number of calls, the count
per method and the SHA-256 of the rendered lines (method, then every argument,
buffers as storage number + offset).  The GPU driver tests compare values bit
for bit with the oracles; this one notices a call that moved, changed an
argument or went to another buffer, on a machine without a GPU.

The golden was recorded from the single-file drivers the package replaced
(tests/golden/make_driver_calls.py says how).
"""
import json
from pathlib import Path

import pytest

import _driver_trace as dt

GOLDEN = Path(__file__).resolve().parent / "golden" / "driver_calls.json"


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_golden_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(dt.CASES)


@pytest.mark.parametrize("name", list(dt.CASES))
def test_driver_calls(golden, tmp_path, name):
    phases = dt.trace(name)
    want = golden[name]
    got = {p: dt.summary(lines) for p, lines in phases.items()}
    if got == want:
        return
    dump = tmp_path / (name.replace("/", "__") + ".txt")
    dump.write_text(dt.text(phases))
    first = next((p for p in want if got.get(p) != want[p]), None) or \
        next(p for p in got if p not in want)
    g, w = got.get(first, {}), want.get(first, {})
    diff = {m: (w.get("methods", {}).get(m, 0), g.get("methods", {}).get(m, 0))
            for m in sorted(set(w.get("methods", {})) | set(g.get("methods", {})))
            if w.get("methods", {}).get(m, 0) != g.get("methods", {}).get(m, 0)}
    pytest.fail(f"{name}: phase {first!r} differs from the golden: {w.get('calls')} calls "
                f"recorded, {g.get('calls')} made; per method (golden, now): {diff or 'equal'}; "
                f"digest {'equal' if g.get('sha256') == w.get('sha256') else 'differs'}.  "
                f"The new trace is in {dump}")


def test_every_branch_is_reached():
    """Every layer kind is driven in inference, in training and backward, and
    the kinds whose backward depends on a layer below both with and without
    one (layer 0)."""
    from tensorium_amd import darknet as dn
    infer, train, at0, above = set(), set(), set(), set()
    for case in dt.CASES.values():
        net = dn.Network(dn.parse_cfg(case["cfg"]), rnn=True)
        for l in net.layers:
            (train if case["train"] else infer).add(l.kind)
            if case["train"]:
                (above if l.index else at0).add(l.kind)
    kinds = {"convolutional", "shortcut", "route", "upsample", "yolo", "maxpool", "local_avgpool",
             "connected", "dropout", "softmax", "cost", "logistic", "lstm", "rnn"}
    assert infer == kinds and train == kinds
    both = {"convolutional", "maxpool", "local_avgpool", "connected", "dropout", "softmax", "cost",
            "logistic", "lstm", "rnn"}
    assert both <= at0 and both <= above
