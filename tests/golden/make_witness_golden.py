"""Writes tests/golden/witness.json: per watch of every search of tests/witness_cases.py, the first
depth at which it held, the number of states holding it there and the holder with the smallest
fingerprint (hi, lo, packed state, trace length), as tests/hostcheck/witnesscheck.cpp computes them
on the host (exact state equality, the holder chosen two independent ways, disagree 0). The
engine's witnesses are tested against this file.

    python tests/golden/make_witness_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import witness_cases  # noqa: E402


def compute(exe=None):
    exe = exe or witness_cases.witnesscheck_build("plain")
    out = {}
    for name in witness_cases.CASES:
        _, settings, _ = witness_cases.case(name)
        row = witness_cases.witnesscheck_run(exe, name)
        assert row["disagree"] == 0 and row["errors"] == 0, row
        out[name] = {"watches": [w.name for w in settings.watches()], "per_depth": row["per_depth"],
                     "witnesses": row["witnesses"]}
    return out


if __name__ == "__main__":
    with open(witness_cases.GOLDEN, "w") as f:
        rows = compute()
        f.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(rows[k], sort_keys=True)) for k in sorted(rows)) + "\n}\n")
    print("wrote", witness_cases.GOLDEN)
