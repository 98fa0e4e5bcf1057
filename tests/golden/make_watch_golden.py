"""Writes tests/golden/watch.json: the census of every watched search of tests/watch_cases.py as
tests/hostcheck/watchcheck.cpp computes it on the host (exact state equality, the watches
evaluated two independent ways, mismatch 0). The engine's census is tested against this file.
The cases of watch_cases.ORACLE_CASES are counted by the CPU oracle instead (`bfs --watch`).

    python tests/golden/make_watch_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_util  # noqa: E402
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
    out.update(compute_oracle())
    return out


def compute_oracle():
    """mp_mut1_watch_logs: the oracle's per-depth counts of the four watches. A fifth watch, asked
    only here, counts the states in which two servers hold different CHOSEN commands in one slot
    (slotValid's conflict branch); the case exists to reach them, so there must be some."""
    args = list(watch_cases.MUT_ORACLE_ARGS)
    for w in watch_cases.MUT_WATCHES + ["CHOSEN_CONFLICT"]:
        args += ["--watch", w]
    r = oracle_util.run("bfs", args, timeout=600)
    census, conflict = r["watch_counts"][:-1], r["watch_counts"][-1]
    assert r["end"] == "SPACE_EXHAUSTED" and sum(conflict) > 0, (r["end"], conflict)
    # a conflicting-chosen state has an invalid slot: the conflict states are among those counted
    assert all(c <= v for c, v in zip(conflict, census[0])), (conflict, census[0])
    return {"mp_mut1_watch_logs": {"watches": watch_cases.MUT_WATCHES, "per_depth": r["per_depth"], "census": census,
                                   "true": [sum(v) for v in census], "chosen_conflict": conflict,
                                   "source": "oracle bfs " + " ".join(args)}}


if __name__ == "__main__":
    with open(watch_cases.GOLDEN, "w") as f:
        rows = compute()
        f.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(rows[k], sort_keys=True)) for k in sorted(rows)) + "\n}\n")
    print("wrote", watch_cases.GOLDEN)
