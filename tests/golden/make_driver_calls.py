"""Generate tests/golden/driver_calls.json: per case and phase of
tests/_driver_trace.py the number of backend calls the darknet drivers make,
the count per method and the SHA-256 of the rendered lines.

The file pins the call sequence of the drivers as they were before they were
split into the ``tensorium_amd/darknet`` package: it was recorded from that
commit's single ``darknet.py`` with the device literal changed and nothing
else, and the package has to match it as recorded.  Regenerate it only when a
change is meant to alter the sequence, and compare the full traces of the two
trees first:

    python tests/golden/make_driver_calls.py --dump DIR    (in each tree)
    diff -r DIR_A DIR_B

Run:  python tests/golden/make_driver_calls.py [--dump DIR]   (deterministic)
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import _driver_trace as dt  # noqa: E402

OUT = HERE / "driver_calls.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="DIR", help="write every case's full trace under DIR")
    ap.add_argument("--out", default=str(OUT))
    args = ap.parse_args()
    rows = []
    for name in dt.CASES:
        phases = dt.trace(name)
        if args.dump:
            p = Path(args.dump) / (name.replace("/", "__") + ".txt")
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_text(dt.text(phases))
        row = json.dumps({p: dt.summary(lines) for p, lines in phases.items()},
                         separators=(",", ":"))
        rows.append(f"{json.dumps(name)}:{row}")
    Path(args.out).write_text("{\n" + ",\n".join(rows) + "\n}\n")
    print(f"{len(rows)} cases -> {args.out}")


if __name__ == "__main__":
    main()
