"""The searches whose watches ask for a witness (SearchSettings.addWatch(p, witness=True)), shared
by the fixture generator (tests/golden/make_witness_golden.py), the CPU tests
(test_watch_witness.py) and the engine tests (test_gpu_watch_witness.py): the six watched searches
of tests/watch_cases.py with every watch wanting a witness, and one PingPongIR search with a watch
no reachable state holds and a watch that holds on the start state. tests/golden/witness.json holds,
per watch, what tests/hostcheck/witnesscheck.cpp computed on the host: the first depth, the number
of states holding the watch there, and the holder with the smallest fingerprint."""
import json
import os
import subprocess

import watch_cases
from dslabs_amd import CLIENTS_DONE, RESULTS_OK, SearchSettings
from dslabs_amd.protocols import PingPongIR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "witness.json")
SRC = os.path.join(HERE, "hostcheck", "witnesscheck.cpp")

PP_EXTRA = ["results>=11 (unreachable)", "results==0 (the start state)", "CLIENTS_DONE"]


def _pingpong_extra():
    p = PingPongIR(1, 10)
    n = p.length("client1", "_results")
    s = SearchSettings().addInvariant(RESULTS_OK).addPrune(CLIENTS_DONE)
    s.table_log2_slots = 20
    s.addWatch(n >= 11).addWatch(n == 0).addWatch(CLIENTS_DONE)
    return p, s, None


CASES = dict(watch_cases.CASES)
CASES["pp_1c10p_extra"] = _pingpong_extra


def with_witnesses(settings, which=None):
    """The same settings with a witness requested for every watch (or those of `which`)."""
    s = settings.clone()
    ws = s.watches()
    s.clearWatches()
    for i, w in enumerate(ws):
        s.addWatch(w, witness=which is None or i in which)
    return s


def case(name):
    """(protocol, settings with every watch wanting a witness, start state or None)"""
    proto, settings, state = CASES[name]()
    return proto, with_witnesses(settings), state


def gold(name):
    with open(GOLDEN) as f:
        return json.load(f)[name]


def gold_state(name, w):
    """The fixture's witness of watch w as packed bytes, or None."""
    row = gold(name)["witnesses"][w]
    return bytes.fromhex(row["state"]) if row["first_depth"] >= 0 else None


def witnesscheck_build(kind="plain"):
    out = os.path.join(HERE, "hostcheck", "_build", "witnesscheck_" + kind)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    deps = [SRC, watch_cases.SRC] + [os.path.join(dp, f) for d in ("dslabs_amd/csrc", "include")
                                     for dp, _, fs in os.walk(os.path.join(ROOT, d)) for f in fs]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        flags = ["-O2"] if kind == "plain" else \
            ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
        subprocess.run([watch_cases.HIPCC, "-std=c++17", "-Wno-unused-result", "-Wno-pass-failed", "-Wno-unused-function"]
                       + flags + ["-o", out, SRC], check=True)
    return out


def witnesscheck_run(exe, name, tmp_dir=None):
    proto, settings, state = case(name)
    return watch_cases.watchcheck_run(exe, name, proto, settings, state, tmp_dir)
