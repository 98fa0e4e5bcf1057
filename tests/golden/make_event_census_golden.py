"""Writes tests/golden/event_census.json: for every search of tests/event_cases.py, the event
census as tests/hostcheck/eventcheck.cpp computes it on the host (a breadth-first walk with exact
state equality; no fingerprint, no table): per_depth, the successors total, the rows as sparse
cells [cls, to, events, noops, exceptions, fresh], and the terminal the search ended on. The
engine's census is tested against this file. pb_stage2 starts from pb_initview's terminal, so the
cases run in CASES' order.

    python tests/golden/make_event_census_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import event_cases  # noqa: E402


def compute(exe=None, names=None):
    exe = exe or event_cases.eventcheck_build("plain")
    out = {}
    for name in names or event_cases.CASES:
        goal = out["pb_initview"]["terminal"] if name == "pb_stage2" and "pb_initview" in out else None
        row = event_cases.eventcheck_run(exe, name, goal)
        assert row["errors"] == 0, row
        out[name] = {k: row[k] for k in ("end", "initial_depth", "per_depth", "successors", "classes", "nodes", "rows",
                                         "terminal")}
    return out


if __name__ == "__main__":
    rows = compute()
    with open(event_cases.GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(rows[k], sort_keys=True, separators=(",", ":")))
                                   for k in sorted(rows)) + "\n}\n")
    print("wrote", event_cases.GOLDEN)
