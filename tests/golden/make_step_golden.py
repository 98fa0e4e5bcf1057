"""Writes tests/golden/step.json: for every search of tests/step_cases.py, what
tests/hostcheck/stepcheck.cpp computes on the host (a breadth-first walk with exact state equality;
no fingerprint decides identity, no table; every step invariant evaluated twice on every judged
edge, the two evaluations compared): the end, per_depth, the judged edges per level and the
violation with its counts and the three diagnostics of the violating level. The engine's step
invariants are tested against this file.

The conditions the cases are chosen for are asserted here, not left to chance.

    python tests/golden/make_step_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import step_cases  # noqa: E402

KEYS = ("end", "pred_index", "terminal_depth", "step_terminal", "initial_depth", "per_depth", "edges", "violation")


def compute(exe=None, names=None):
    exe = exe or step_cases.stepcheck_build("plain")
    out = {}
    for name in names or step_cases.CASES:
        row = step_cases.stepcheck_run(exe, name, rows=out)  # in CASES' order: a later case may start from an earlier answer
        assert row["errors"] == 0 and row["mismatches"] == 0, row
        out[name] = {k: row[k] for k in KEYS}
    return out


def check_conditions(rows):
    """What the cases must exhibit (ISSUE: Cases)."""
    for name, (_, _, kind) in step_cases.CASES.items():
        assert (rows[name]["violation"] is not None) == (kind == "viol"), (name, kind)
    viols = {n: r["violation"] for n, r in rows.items() if r["violation"]}
    assert any(v["edges"] >= 2 for v in viols.values()), "no violating level with at least 2 violating edges"
    assert any(v["both"] > 0 for v in viols.values()), \
        "no successor reached by both a violating and a non-violating edge"
    assert any(v["shallower"] > 0 for v in viols.values()), \
        "no violating edge to a state first discovered at a shallower depth"
    # the named ones
    assert viols["mp_c5_d8_ir_heard"]["both"] > 0 and viols["mp_c5_d8_ir_heard"]["shallower"] > 0
    assert viols["mp_c5_d8_ir_active"]["shallower"] > 0 and viols["mp_c5_d8_ir_active"]["depth"] == 7
    # eight step invariants, several of them violated by one edge
    e = viols["mp_c5_d8_ir_eight"]
    assert len(e["per_invariant"]) == 8 and sum(1 for c in e["per_invariant"] if c) >= 2
    assert sum(e["per_invariant"]) > e["edges"]
    # ... whose eighth tree (every leaf kind) holds, and is not vacuous: its antecedent fires on
    # edges of a level that case judges
    f = viols["mp_c5_d8_ir_fires"]
    assert e["per_invariant"][7] == 0 and f["edges"] > 0 and f["depth"] <= e["depth"]
    # named network leaves decided by dropped records alone
    for form in ("pb_dropped", "pb_dropped_ir"):
        assert viols[form + "_viol"]["index"] == 1 and viols[form + "_viol"]["edges"] == rows[form + "_viol"]["edges"][0]
        assert len(rows[form + "_hold"]["edges"]) >= 2
    # the priorities: a state invariant and an exception outrank the step violation, a goal does not
    assert rows["prio_inv"]["end"] == 1 and not rows["prio_inv"]["step_terminal"]
    assert rows["prio_inv"]["terminal_depth"] == viols["prio_inv"]["depth"]
    assert rows["prio_goal"]["end"] == 1 and rows["prio_goal"]["step_terminal"]
    assert rows["minitest_viol"]["end"] == 0 and not rows["minitest_viol"]["step_terminal"]
    # every protocol family has a step invariant that holds and one that is violated
    for fam in ("lab0", "kv_", "sipaxos", "synth", "mp_", "pb_"):
        kinds = {k for n, (_, _, k) in step_cases.CASES.items() if n.startswith(fam)}
        assert kinds == {"hold", "viol"}, (fam, kinds)


if __name__ == "__main__":
    rows = compute()
    check_conditions(rows)
    with open(step_cases.GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(rows[k], sort_keys=True, separators=(",", ":")))
                                   for k in sorted(rows)) + "\n}\n")
    print("wrote", step_cases.GOLDEN)
