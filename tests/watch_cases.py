"""The watched searches (SearchSettings.addWatch) shared by the host check's fixture generator
(tests/golden/make_watch_golden.py), the CPU tests (test_watch.py) and the engine tests
(test_gpu_watch.py): each case is a protocol, its settings with the watches added, and -- in
tests/golden/watch.json -- the census tests/hostcheck/watchcheck.cpp computed for it on the host.
The oracle's anchors (first depth, states holding the watch there) are ANCHORS below: what the
committed oracle answers to `bfs --goal P --finish-level`."""
import json
import os
import subprocess
import tempfile

import argmap
from dslabs_amd import CLIENTS_DONE, NONE_DECIDED, RESULTS_OK, SearchSettings, _lib
from dslabs_amd.protocols import PB, MultiPaxos, MultiPaxosIR, PingPongIR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "watch.json")
SRC = os.path.join(HERE, "hostcheck", "watchcheck.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def gold(name):
    with open(GOLDEN) as f:
        return json.load(f)[name]


def fixture(fname, name):
    with open(os.path.join(HERE, "golden", fname + ".json")) as f:
        return json.load(f)[name]


def _settings(table_log2=20):
    s = SearchSettings()
    s.table_log2_slots = table_log2
    return s


# ---- lab0: PingPongIR, 1 client x 10 pings, exhaustive with CLIENTS_DONE pruned -------------------------
PP_NAMES = ["CLIENTS_DONE", "results>=5", "!(results>=5)", "results>=0", "Pong(value>=5)", "Pong>=5 and !(results>=5)",
            "results==0", "Pong to client1(value>=9)"]


def pingpong_watches(p):
    n = p.length("client1", "_results")
    pong = p.message("PongReply")
    pong5 = pong.where(pong.field("value") >= 5)
    to = p.message("PongReply", to="client1")
    return [CLIENTS_DONE, n >= 5, (n >= 5).negate(), n >= 0, pong5, pong5.and_((n >= 5).negate()), n == 0,
            to.where(to.field("value") >= 9)]


def _pingpong():
    p = PingPongIR(1, 10)
    s = _settings().addInvariant(RESULTS_OK).addPrune(CLIENTS_DONE)
    for w in pingpong_watches(p):
        s.addWatch(w)
    return p, s, None


def _pingpong_goal():
    """lab0_1c10p_goal with the goal also a watch (the engine's find-mode case)."""
    p = PingPongIR(1, 10)
    s = _settings().addInvariant(RESULTS_OK).addGoal(CLIENTS_DONE).addWatch(CLIENTS_DONE)
    return p, s, None


# ---- lab3: mp_c5_d8, the fixture's three invariants, maxDepth 8 ------------------------------------------
MP_NAMED = ["hasStatus:server2:1:ACCEPTED", "!NONE_DECIDED", "hasStatus:server2:1:CHOSEN", "clientDone:client1",
            "hasStatus:server3:2:CHOSEN", "and(clientDone:client1,hasStatus:server3:1:CHOSEN)", "CLIENTS_DONE"]
STATUS = {"EMPTY": 0, "ACCEPTED": 1, "CHOSEN": 2}


def _mp_settings(proto):
    s = _settings().addInvariant(RESULTS_OK).addInvariant(proto.predicate("LOGS_CONSISTENT_ALL_SLOTS"))
    return s.addInvariant(proto.predicate("APPENDS_LINEARIZABLE")).maxDepth(8)


def _mp_named(proto):
    s = _mp_settings(proto)
    for name in MP_NAMED:
        s.addWatch(argmap.predicate(proto, name))
    return proto, s, None


def has_status(mp, server, slot, status):
    """hasStatus(a, i, s) over MultiPaxosIR's log (tests/test_gpu_field_predicates.py has_status)."""
    return mp.field(server, "log", slot - 1).bits(0, 2) == STATUS[status]


# the generic case's watches: (name, the MP_NAMED watch it restates or None)
MP_GENERIC = [("field hasStatus:server2:1:ACCEPTED", "hasStatus:server2:1:ACCEPTED"),
              ("field hasStatus:server2:1:CHOSEN", "hasStatus:server2:1:CHOSEN"),
              ("field hasStatus:server3:2:CHOSEN", "hasStatus:server3:2:CHOSEN"),
              ("Decision(slot == 1)", None), ("P2a from server2", None),
              ("Decision(slot == 1) or field hasStatus:server2:1:CHOSEN", None),
              ("hasStatus:server2:1:CHOSEN", "hasStatus:server2:1:CHOSEN"), ("CLIENTS_DONE", "CLIENTS_DONE")]


def _mp_generic():
    mp = MultiPaxosIR(3, 2, "append-xy")
    dec = mp.message("Decision")
    dec1 = dec.where(dec.field("slot") == 1)
    chosen = has_status(mp, "server2", 1, "CHOSEN")
    s = _mp_settings(mp)
    for w in (has_status(mp, "server2", 1, "ACCEPTED"), chosen, has_status(mp, "server3", 2, "CHOSEN"), dec1,
              mp.message("P2a", frm="server2").where(), dec1.or_(chosen), mp.predicate("hasStatus:server2:1:CHOSEN"),
              CLIENTS_DONE):
        s.addWatch(w)
    return mp, s, None


# ---- lab2: PB's named network predicate (kNetPreds) and its raw-message restatement -----------------------
def _pb():
    pb = PB(2, 1, "putget")
    m = pb.raw_message("ViewReply")
    s = _settings().addInvariant(RESULTS_OK).maxDepth(6)
    s.addWatch(pb.predicate("hasViewReply:1")).addWatch(m.where(m.raw_field(60, 4) == 2, m.raw_field(0, 4) >= 1))
    s.addWatch(pb.predicate("hasViewReply:2").negate()).addWatch(NONE_DECIDED)
    return pb, s, None


CASES = {
    "pp_1c10p_8w": _pingpong,
    "pp_1c10p_goal": _pingpong_goal,
    "mp_c5_d8_named": lambda: _mp_named(MultiPaxos(3, 2, "append-xy")),
    "mpir_c5_d8_named": lambda: _mp_named(MultiPaxosIR(3, 2, "append-xy")),
    "mpir_c5_d8_generic": _mp_generic,
    "pb_2s1c_d6": _pb,
}

# ---- lab3 with the adopt-chosen-only mutant: the log predicates false, counted by the ORACLE ---------------
# No invariants, so the search goes on past the first violation (depth 8, no majority) into states
# where two servers hold different CHOSEN commands in a slot (depth 10): slotValid's other false branch.
# Its census in watch.json is the oracle's (`bfs --watch`, every predicate evaluated in full), not
# watchcheck's: tests/golden/make_watch_golden.py. APPENDS_LINEARIZABLE is not yet false by depth 10.
MUT_WATCHES = ["!LOGS_CONSISTENT_ALL_SLOTS", "!slotValid:1", "!slotValid:2", "!APPENDS_LINEARIZABLE"]
MUT_ORACLE_ARGS = ["--proto", "multipaxos", "--workload", "append-xy", "--mutant", "adopt-chosen-only",
                   "--max-depth", "10"]


def mut1_watch_logs(cls=MultiPaxos):
    """(protocol, settings, None) of mp_mut1_watch_logs on MultiPaxos or MultiPaxosIR."""
    proto = cls(3, 2, "append-xy", mutant="adopt-chosen-only")
    s = _settings(22).maxDepth(10)
    for name in MUT_WATCHES:
        s.addWatch(argmap.predicate(proto, name))
    return proto, s, None


ORACLE_CASES = {"mp_mut1_watch_logs": mut1_watch_logs}

# (case, watch index) -> (first depth, states holding the watch there): the committed oracle's
# `bfs --goal P --finish-level` (max_depth of the result, num_terminals), ORACLE_ARGS below
ANCHORS = {
    ("pp_1c10p_8w", 0): (20, 1),
    ("pb_2s1c_d6", 0): (1, 2),
    ("mp_c5_d8_named", 0): (2, 2), ("mp_c5_d8_named", 1): (4, 4), ("mp_c5_d8_named", 2): (4, 4),
    ("mp_c5_d8_named", 3): (4, 2), ("mp_c5_d8_named", 4): (5, 4), ("mp_c5_d8_named", 5): (5, 2),
    ("mp_c5_d8_named", 6): (8, 8),
}
_MP = ["--proto", "multipaxos", "--workload", "append-xy"]
_FIN = ["--finish-level", "--max-terminals", "0"]
ORACLE_ARGS = {
    ("pp_1c10p_8w", 0): ["--proto", "pingpong", "--clients", "1", "--pings", "10", "--goal", "CLIENTS_DONE"] + _FIN,
    ("pb_2s1c_d6", 0): ["--proto", "pb", "--goal", "hasViewReply:1"] + _FIN,
}
for _k, _name in enumerate(MP_NAMED):
    ORACLE_ARGS[("mp_c5_d8_named", _k)] = _MP + ["--goal", _name, "--max-depth", "9"] + _FIN


def case(name):
    """(protocol, settings with the watches, start state or None)"""
    return CASES[name]()


# ---- tests/hostcheck/watchcheck.cpp ------------------------------------------------------------------------
def watchcheck_build(kind="plain"):
    out = os.path.join(HERE, "hostcheck", "_build", "watchcheck_" + kind)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    deps = [SRC] + [os.path.join(dp, f) for d in ("dslabs_amd/csrc", "include") for dp, _, fs in os.walk(os.path.join(ROOT, d))
                    for f in fs]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        flags = ["-O2"] if kind == "plain" else \
            ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
        subprocess.run([HIPCC, "-std=c++17", "-Wno-unused-result", "-Wno-pass-failed"] + flags + ["-o", out, SRC], check=True)
    return out


def blob(proto, settings, state=None):
    """What watchcheck reads: dsl_protocol_desc, dsl_settings, then the watches as dsl_set_watches
    takes them (n, n_pool, 8 + 48 dsl_predicate), the dropped records and the start state."""
    st = state if state is not None else proto.initial_state()
    _, w, n, pool, n_pool = settings._encode_watches(st)
    w = w if w is not None else (_lib.dsl_predicate * _lib.DSL_MAX_WATCHES)()
    pool = pool if pool is not None else (_lib.dsl_predicate * _lib.DSL_MAX_POOL)()
    i32 = lambda v: int(v).to_bytes(4, "little", signed=True)  # noqa: E731
    b = bytes(proto.desc()) + bytes(settings._encode(st)) + i32(n) + i32(n_pool) + bytes(w) + bytes(pool)
    dropped = list(st._dropped)
    packed = st.packed if state is not None and st.packed is not None else b""
    b += i32(len(dropped)) + i32(st.depth() if packed else 0) + i32(len(packed)) + i32(0)
    b += b"".join(int(r).to_bytes(8, "little") for r in dropped) + packed
    return b


def watchcheck_run(exe, name, proto, settings, state=None, tmp_dir=None):
    with tempfile.NamedTemporaryFile("wb", suffix=".blob", delete=False, dir=tmp_dir) as f:
        f.write(blob(proto, settings, state))
        path = f.name
    try:
        p = subprocess.run([exe, name, path], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr, p.stderr
    return json.loads(p.stdout.splitlines()[-1])

