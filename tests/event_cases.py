"""The searches of the event census (SearchSettings.eventCensus), shared by the fixture generator
(tests/golden/make_event_census_golden.py), the CPU tests (test_event_census.py) and the engine
tests (test_gpu_event_census.py): one or more per device protocol, from the smallest committed
fixtures, and -- in tests/golden/event_census.json -- the rows tests/hostcheck/eventcheck.cpp
computed for each on the host with exact state equality.

A case is (oracle-style args, fixture to tie per_depth to or None). ``args`` is what tests/argmap.py
turns into a protocol and settings; FIXTURE names a committed per_depth the host walk must
reproduce: the whole vector, or -- for a case that only adds --max-depth to a fixture's args, in a
search without terminals -- its first max-depth + 1 entries."""
import json
import os
import subprocess
import tempfile

import argmap
import watch_cases
from dslabs_amd.search import SearchState

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "event_census.json")
SRC = os.path.join(HERE, "hostcheck", "eventcheck.cpp")

_PP = ["--inv", "RESULTS_OK", "--prune", "CLIENTS_DONE"]
_LAB0 = lambda proto, clients: ["--proto", proto, "--clients", str(clients), "--pings", "10"] + _PP  # noqa: E731
_KV = ["--clients", "2", "--workload", "diffkey3"] + _PP
_MP = ["--workload", "append-xy", "--inv", "RESULTS_OK", "--inv", "LOGS_CONSISTENT_ALL_SLOTS", "--inv",
       "APPENDS_LINEARIZABLE", "--max-depth", "8"]
_PB = ["--servers", "2", "--clients", "1", "--workload", "putget"]
_PB15 = _PB + ["--inv", "RESULTS_OK", "--prune", "CLIENTS_DONE", "--prune", "hasViewReply:4"]
INITVIEW = ["--proto", "pb"] + _PB + [
    "--prune", "hasViewReply:3", "--prune", "and(hasViewReply:2,!hasViewReply:2:1:2)", "--network-off", "--active",
    "viewserver", "--link", "server1,server2", "--link", "server2,server1", "--goal",
    "and(viewRepliesSent:2:1:2:server1+server2+client1,!hasViewReply:3)"]

# name -> (args, (fixture file, fixture name) or None)
CASES = {
    "lab0_1c10p_exhaustive": (_LAB0("pingpong", 1), ("lab0", "lab0_1c10p_exhaustive")),
    "lab0_1c10p_exhaustive_ir": (_LAB0("pingpong_ir", 1), ("lab0", "lab0_1c10p_exhaustive")),
    "lab0_2c10p_exhaustive": (_LAB0("pingpong", 2), ("lab0", "lab0_2c10p_exhaustive")),
    "lab0_2c10p_exhaustive_ir": (_LAB0("pingpong_ir", 2), ("lab0", "lab0_2c10p_exhaustive")),
    # deliverTimers(client2, False): the silenced timers' cell stays zero
    "lab0_2c3p_notimers": (["--proto", "pingpong", "--clients", "2", "--pings", "3"] + _PP + ["--no-timers", "client2"],
                           ("lab0", "lab0_2c3p_notimers")),
    "kv_test09": (["--proto", "amokv"] + _KV, ("amokv", "kv_test09_exhaustive")),
    "kv_test09_ir": (["--proto", "amokv_ir"] + _KV, ("amokv", "kv_test09_exhaustive")),
    "sipaxos_2p3a_d6": (["--proto", "sipaxos", "--proposers", "2", "--acceptors", "3", "--values", "a,b", "--inv", "Integrity",
                         "--inv", "Agreement", "--max-depth", "6"], ("sipaxos", "sipaxos_2p3a_d6")),
    # the synthetic C3 (5 nodes, 64 values) to depth 3: a few thousand states
    "synth_c3_d3": (["--proto", "synthetic", "--inv", "NOT_ALL_MAX", "--max-depth", "3"], ("synthetic", "synth_c3_d5")),
    # MiniTest: a's Foo handler throws -- a non-zero `exceptions` cell, and the search ends on it
    "minitest": (["--proto", "minitest"], None),
    "mp_c5_d8": (["--proto", "multipaxos"] + _MP, ("multipaxos", "mp_c5_d8")),
    "mp_c5_d8_ir": (["--proto", "multipaxos_ir"] + _MP, ("multipaxos", "mp_c5_d8")),
    "pb_2s1c_d7": (["--proto", "pb"] + _PB15 + ["--max-depth", "7"], ("pb", "pb_2s1c_d15")),
    "pb_2s1c_d7_ir": (["--proto", "pb_ir"] + _PB15 + ["--max-depth", "7"], ("pb", "pb_2s1c_d15")),
    # initView's search: most links are closed, so most records of a state are no events; it ends
    # with a goal, whose level is a completed level
    "pb_initview": (INITVIEW, ("pb", "pb_initview_search")),
}
# linkActive(a, b, False) and deliverTimers(node, False) in one search (case() below)
CASES["mp_c5_d6_cut"] = (["--proto", "multipaxos"] + _MP[:-1] + ["6"], None)
# the second stage: from pb_initview's goal state (initial_depth 11) with part of its network
# dropped -- records that are no events -- five levels of the C4 search
CASES["pb_stage2"] = (["--proto", "pb"] + _PB15 + ["--max-depth", "16"], None)

# cells that must be zero in every row: (class name, address)
ZERO_CELLS = {
    "lab0_2c3p_notimers": [("PingTimer", "client2")],
    "mp_c5_d6_cut": [("PaxosRequest", "server1"), ("TickTimer", "server1"), ("ClientTimer", "client2")],
}


def gold(name=None):
    with open(GOLDEN) as f:
        g = json.load(f)
    return g if name is None else g[name]


def fixture_per_depth(name):
    """The committed oracle per_depth this case's host walk must reproduce, or None."""
    args, fx = CASES[name]
    if fx is None:
        return None
    with open(os.path.join(HERE, "golden", fx[0] + ".json")) as f:
        row = json.load(f)[fx[1]]
    pd = row["per_depth"]
    depth_of = lambda a: int(a[a.index("--max-depth") + 1]) if "--max-depth" in a else None  # noqa: E731
    if depth_of(args) != depth_of(row["args"]):
        pd = pd[:depth_of(args) + 1]
    return pd


def stage2_start(proto, goal_hex, depth):
    """pb_stage2's start: the first stage's goal state with its pending messages dropped and those
    from the ViewServer and server1 pending again (the others stay dropped: part of network() for
    the predicates, no events)."""
    st = SearchState(proto, bytes.fromhex(goal_hex), depth)
    st.dropPendingMessages()
    st.undropMessagesFrom("viewserver")
    st.undropMessagesFrom("server1")
    return st


def case(name, goal=None):
    """(protocol, settings without the census, start state or None). ``goal``: pb_stage2's first
    stage terminal {"depth", "state"} (default: the committed fixture's)."""
    args, _ = CASES[name]
    proto = argmap.protocol(args)
    s = argmap.settings(args, proto, table_log2=20)
    state = None
    if name == "mp_c5_d6_cut":
        s.linkActive("client1", "server1", False).linkActive("client2", "server1", False)  # the only senders of a PaxosRequest
        s.deliverTimers("server1", False).deliverTimers("client2", False)
    if name == "pb_stage2":
        goal = goal or gold("pb_initview")["terminal"]
        state = stage2_start(proto, goal["state"], goal["depth"])
    return proto, s, state


# ---- tests/hostcheck/eventcheck.cpp ---------------------------------------------------------------------
def eventcheck_build(kind="plain"):
    out = os.path.join(HERE, "hostcheck", "_build", "eventcheck_" + kind)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    deps = [SRC] + [os.path.join(dp, f) for d in ("dslabs_amd/csrc", "include") for dp, _, fs in os.walk(os.path.join(ROOT, d))
                    for f in fs]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        flags = ["-O2"] if kind == "plain" else \
            ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
        subprocess.run([watch_cases.HIPCC, "-std=c++17", "-Wno-unused-result", "-Wno-pass-failed", "-Wno-unused-function"]
                       + flags + ["-o", out + ".tmp", SRC], check=True)
        os.replace(out + ".tmp", out)
    return out


def eventcheck_run(exe, name, goal=None, tmp_dir=None):
    proto, settings, state = case(name, goal)
    with tempfile.NamedTemporaryFile("wb", suffix=".blob", delete=False, dir=tmp_dir) as f:
        f.write(watch_cases.blob(proto, settings, state))
        path = f.name
    try:
        p = subprocess.run([exe, name, path], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr, p.stderr
    return json.loads(p.stdout.splitlines()[-1])


def dense(row_cells, n_classes, n_nodes):
    """A golden row's sparse cells [cls, to, events, noops, exceptions, fresh] as
    SearchResults.eventRows() gives a row: [cls][to] = (events, noops, exceptions, fresh)."""
    out = [[(0, 0, 0, 0) for _ in range(n_nodes)] for _ in range(n_classes)]
    for c, t, *v in row_cells:
        out[c][t] = tuple(v)
    return out


def check_identities(rows, per_depth, successors, whole=True):
    """The census's identities, on the golden and on every engine result. rows: dense rows."""
    cells = [v for row in rows for cls in row for v in cls]
    if whole:  # no level was cut short: the events are the successors
        assert sum(v[0] for v in cells) == successors
    for e, n, x, f in cells:
        assert f <= e - n - x and min(e, n, x, f) >= 0
    for i, row in enumerate(rows):
        if i + 1 < len(per_depth):
            assert sum(v[3] + v[2] for cls in row for v in cls) >= per_depth[i + 1]
