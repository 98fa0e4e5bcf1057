"""Writes tests/golden/watch.json: the census of every watched search of tests/watch_cases.py as
tests/hostcheck/watchcheck.cpp computes it on the host (exact state equality, the watches
evaluated two independent ways, mismatch 0). The engine's census is tested against this file.

    python tests/golden/make_watch_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import watch_cases  # noqa: E402


def compute(exe=None):
    exe = exe or watch_cases.watchcheck_build("plain")
    out = {}
    for name in watch_cases.CASES:
        proto, settings, state = watch_cases.case(name)
        row = watch_cases.watchcheck_run(exe, name, proto, settings, state)
        assert row["mismatch"] == 0 and row["errors"] == 0 and row["search_changed"] == 0, row
        out[name] = {"watches": [w.name for w in settings.watches()], "per_depth": row["per_depth"],
                     "census": row["census"], "true": row["true"]}
    return out


if __name__ == "__main__":
    with open(watch_cases.GOLDEN, "w") as f:
        rows = compute()
        f.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(rows[k], sort_keys=True)) for k in sorted(rows)) + "\n}\n")
    print("wrote", watch_cases.GOLDEN)
