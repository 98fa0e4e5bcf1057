"""The searches with step invariants (SearchSettings.addStepInvariant), shared by the fixture
generator (tests/golden/make_step_golden.py), the CPU tests (test_step.py) and the engine tests
(test_gpu_step.py). A case is a search of tests/event_cases.py -- so the committed event census and
the oracle's per_depth anchor it -- plus step invariants; tests/golden/step.json holds what
tests/hostcheck/stepcheck.cpp computed for each on the host with exact state equality.

CASES: name -> (event case, builder(proto, settings) -> None adding the step invariants (and, for
the priority cases, a state invariant or a goal), "hold" | "viol"). STARTS names the cases that take their
event case's protocol and settings but start elsewhere (a dropped set of their own); the census does
not anchor those."""
import json
import os
import subprocess
import tempfile

import event_cases
import watch_cases
from dslabs_amd import NONE_DECIDED, _lib, new, old
from dslabs_amd.search import SearchState

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "step.json")
SRC = os.path.join(HERE, "hostcheck", "stepcheck.cpp")
CHOSEN = 2


def word(p, addr, w):
    return p.raw_field(addr, 32 * w, 32)


def local(p, addr, w=0):
    """Node-locality: word w of a node changes only under an event delivered to that node."""
    x = word(p, addr, w)
    return p.delivered(to=addr).or_(new(x) == old(x))


# ---- lab0 (hand-written and IR) ---------------------------------------------------------------------------
def _nres(p, c):
    return p.length(c, "_results") if hasattr(p, "length") else p.raw_field(c, 8, 4)


def _pong(p):
    if hasattr(p, "message"):
        return p.message("PongReply").sent()
    m = p.raw_message("PongReply", 32)
    return m.sent(m.raw_field(31, 1) == 1)


def _lab0_hold(p, s):
    for c in p.addresses[1:]:
        s.addStepInvariant(new(_nres(p, c)) >= old(_nres(p, c)))
        s.addStepInvariant(local(p, c))
    # only the server's PingRequest handler adds a PongReply
    s.addStepInvariant(_pong(p).implies(p.delivered("PingRequest", to="pingserver")))
    s.addStepInvariant(p.delivered("PingTimer").implies(_pong(p).negate()))


def _lab0_viol(p, s):
    c = p.addresses[-1]
    s.addStepInvariant(new(_nres(p, c)) >= old(_nres(p, c)))  # holds
    s.addStepInvariant(new(_nres(p, c)) == old(_nres(p, c)))  # broken by the first result
    s.addStepInvariant(p.delivered("PongReply", to=c).implies(new(_nres(p, c)) == old(_nres(p, c))))


# ---- the priority cases (lab0 IR, one client): a state invariant / a goal of the violating level --------
def _prio_inv(p, s):
    n = p.length("client1", "_results")
    s.addInvariant(n < 3)
    s.addStepInvariant(new(n) < 3)


def _prio_goal(p, s):
    n = p.length("client1", "_results")
    s.addGoal(n >= 3)
    s.addStepInvariant(new(n) < 3)


# ---- lab1 (IR) -----------------------------------------------------------------------------------------------
def _kv_hold(p, s):
    for c in ("client1", "client2"):
        s.addStepInvariant(new(p.field(c, "seq")) >= old(p.field(c, "seq")))
        s.addStepInvariant(new(p.length(c, "_results")) >= old(p.length(c, "_results")))
    s.addStepInvariant(p.message("Reply").sent().implies(p.delivered("Request", to="server")))
    s.addStepInvariant(local(p, "server", 0))


def _kv_viol(p, s):
    s.addStepInvariant(new(p.field("client1", "seq")) >= old(p.field("client1", "seq")))
    s.addStepInvariant(new(p.field("server", "amo", 0)) == old(p.field("server", "amo", 0)))


# ---- single-instance Paxos (hand-written: raw fields, csrc/protocols/sipaxos.hpp) -------------------------------
def _sip_hold(p, s):
    for a in ("acceptor1", "acceptor2", "acceptor3"):
        hp = p.raw_field(a, 0, 8)  # highestPrepared
        s.addStepInvariant(new(hp) >= old(hp))
    for q in ("proposer1", "proposer2"):
        pn = p.raw_field(q, 16, 8)  # proposalNumber
        s.addStepInvariant(new(pn) >= old(pn))
    m = p.raw_message("AcceptAck", 32)
    s.addStepInvariant(m.sent(m.raw_field(30, 2) == 3).implies(p.delivered("Accept")))


def _sip_viol(p, s):
    an = p.raw_field("acceptor1", 8, 8)  # accepted.n
    s.addStepInvariant(new(an) >= old(an))
    s.addStepInvariant(new(an) == old(an))


# ---- synthetic C3 ----------------------------------------------------------------------------------------------
def _synth_hold(p, s):
    for a in p.addresses:
        s.addStepInvariant(local(p, a))
    m = p.raw_message("Poke", 32)
    s.addStepInvariant(m.sent(m.raw_field(0, 1) >= 0).implies(p.delivered("SynthTimer")))


def _synth_viol(p, s):
    v = p.raw_field("node1", 0, 16)
    s.addStepInvariant(local(p, "node1"))
    s.addStepInvariant(p.delivered("Poke", to="node1").implies(new(v) == old(v)))


# ---- MiniTest: the exception of the violating level outranks the step violation ----------------------------------
def _mini(p, s):
    foo = p.raw_field("a", 0, 1)
    s.addStepInvariant(new(foo) == old(foo))


# ---- lab3 (hand-written: raw fields, csrc/protocols/multipaxos.hpp; IR: named fields) -------------------------------
def _mp_round(p, sv):
    return p.field(sv, "round") if hasattr(p, "field") else p.raw_field(sv, 0, 4)


def _mp_log(p, sv, slot):
    """(entry, status) of log[slot] (slots from 1)."""
    if hasattr(p, "field"):
        e = p.field(sv, "log", slot - 1)
        return e, e.bits(0, 2)
    e = p.raw_field(sv, 32 + 16 * (slot - 1), 16)
    return e, e.bits(0, 2)


def _mp_slotout(p, sv):
    return p.field(sv, "slotout") if hasattr(p, "field") else p.raw_field(sv, 14, 3)


def _mp_decision_sent(p, slot):
    if hasattr(p, "message"):
        d = p.message("Decision")
        return d.sent(d.field("slot") == slot)
    m = p.raw_message("Decision", 64)
    return m.sent(m.raw_field(61, 3) == 6, m.raw_field(0, 3) == slot)


def _mp_hold(p, s):
    for sv in ("server1", "server2", "server3"):
        s.addStepInvariant(new(_mp_round(p, sv)) >= old(_mp_round(p, sv)))
    for sv in ("server1", "server2"):
        e, st = _mp_log(p, sv, 1)
        s.addStepInvariant((old(st) == CHOSEN).implies(new(e) == old(e)))
        # a Decision for slot 1 is only sent by a server whose log[1] is chosen
        s.addStepInvariant(p.delivered(to=sv).and_(_mp_decision_sent(p, 1)).implies(new(st) == CHOSEN))
    so = [new(_mp_slotout(p, sv)) >= old(_mp_slotout(p, sv)) for sv in ("server1", "server2", "server3")]
    s.addStepInvariant(so[0].and_(so[1]).and_(so[2]))


def _mp_slotout_viol(p, s):
    s.addStepInvariant(new(_mp_round(p, "server1")) >= old(_mp_round(p, "server1")))
    s.addStepInvariant(new(_mp_slotout(p, "server1")) == old(_mp_slotout(p, "server1")))


def _mp_elects(p):
    """server3's Tick starts an election: the first one of the search, by depth 2."""
    return p.delivered("Tick|ClientTimer", to="server3").and_(p.message("P1a").sent())


def _mp_eight(p, s):
    """Eight step invariants, several of them broken by one edge: server1 joins a higher round."""
    f = lambda name: p.field("server1", name)  # noqa: E731
    for name in ("round", "electing", "leader", "p1bvotes"):
        s.addStepInvariant(new(f(name)) == old(f(name)))
    s.addStepInvariant(p.message("P1a", frm="server1").sent().negate())
    s.addStepInvariant(new(f("round")) >= old(f("round")))      # holds
    s.addStepInvariant(new(f("slotout")) >= old(f("slotout")))  # holds
    # all three step leaf kinds and a named leaf in one tree. Its antecedent fires in the judged levels
    # (_mp_fires), and there both leaves of the consequent decide: either one false breaks it.
    r3 = p.field("server3", "round")
    s.addStepInvariant(_mp_elects(p).implies((new(r3) > old(r3)).and_(NONE_DECIDED)))


def _mp_fires(p, s):
    """_mp_eight's antecedent as a step invariant of its own: broken where it fires."""
    s.addStepInvariant(_mp_elects(p).negate())


def _mp_heard(p, s):
    """A reset-style relation: a follower's Tick clears its `heard` flag. The violating level has a
    successor reached by both a violating and a non-violating edge, and a violating edge that leads
    to a state first discovered at a shallower depth."""
    s.addStepInvariant(new(p.field("server2", "heard")) >= old(p.field("server2", "heard")))


def _mp_active(p, s):
    """`active` only rises: broken at depth 7 (1,561 parents) by a leader that steps down, on an edge
    whose successor was first discovered at a shallower depth."""
    s.addStepInvariant(new(p.field("server1", "round")) >= old(p.field("server1", "round")))
    s.addStepInvariant(new(p.field("server2", "active")) >= old(p.field("server2", "active")))


def _mp_done(p, s):
    """A named leaf on the successor: no step finishes both workloads. Broken at depth 8, the level
    of the largest frontier (4,050 parents)."""
    from dslabs_amd import CLIENTS_DONE
    s.addStepInvariant(CLIENTS_DONE.negate())


# ---- lab2 (IR; the hand-written protocol from a staged start with a dropped set) ----------------------------------
def _pb_hold(p, s):
    s.addStepInvariant(new(p.field("viewserver", "vnum")) >= old(p.field("viewserver", "vnum")))
    for sv in ("server1", "server2"):
        s.addStepInvariant(new(p.field(sv, "vnum")) >= old(p.field(sv, "vnum")))
    s.addStepInvariant(p.message("ViewReply").sent().implies(p.delivered(to="viewserver")))
    s.addStepInvariant(local(p, "client1"))


def _pb_viol(p, s):
    s.addStepInvariant(new(p.field("viewserver", "vnum")) >= old(p.field("viewserver", "vnum")))
    s.addStepInvariant(new(p.field("viewserver", "vnum")) == old(p.field("viewserver", "vnum")))


def _pb2_hold(p, s):
    vn = p.raw_field("viewserver", 0, 4)
    s.addStepInvariant(new(vn) >= old(vn))
    s.addStepInvariant(local(p, "viewserver"))
    s.addStepInvariant(local(p, "client1", 1))


def _pb2_viol(p, s):
    w0 = word(p, "client1", 0)
    s.addStepInvariant(local(p, "client1"))
    s.addStepInvariant(new(w0) == old(w0))


# ---- named leaves that read the network, from starts whose ViewReplies are in the dropped set only --------------
def _pbd_hold(p, s):
    """hasViewReply on the successor: true only through the dropped records, which are part of
    network() on every successor."""
    s.addStepInvariant(p.predicate("hasViewReply:1:1:-1"))
    s.addStepInvariant(p.predicate("hasViewReply:1"))
    vn = p.field("viewserver", "vnum") if hasattr(p, "field") else p.raw_field("viewserver", 0, 4)
    s.addStepInvariant(p.delivered(to="server1").and_(new(vn) >= old(vn)).implies(p.predicate("hasViewReply:1:1:-1")))


def _pbd_viol(p, s):
    s.addStepInvariant(p.predicate("hasViewReply:1"))                # holds
    s.addStepInvariant(p.predicate("hasViewReply:1:1:-1").negate())  # broken by every edge, by a dropped record


def _pb_dropped_start(proto, rows=None):
    """The hand-written PB: initView's goal state with every pending message dropped and server1's
    pending again -- the ViewServer's ViewReplies stay in the dropped set only."""
    goal = event_cases.gold("pb_initview")["terminal"]
    st = SearchState(proto, bytes.fromhex(goal["state"]), goal["depth"])
    st.dropPendingMessages()
    st.undropMessagesFrom("server1")
    return st


def _pbir_dropped_start(proto, rows=None):
    """The IR protocol: the successor of the ViewServer's first view change (pb_2s1c_d7_ir_viol's
    reported state, from this file's own walk) with every pending message dropped: the only events
    left are timers, and the ViewReply for View(1, server1, null) is a dropped record."""
    v = (rows if rows is not None and "pb_2s1c_d7_ir_viol" in rows else gold())["pb_2s1c_d7_ir_viol"]["violation"]
    st = SearchState(proto, bytes.fromhex(v["state"]), v["depth"])
    st.dropPendingMessages()
    return st


# name -> start(proto, rows computed so far or None) for the cases that do not start where their event case does
STARTS = {"pb_dropped_hold": _pb_dropped_start, "pb_dropped_viol": _pb_dropped_start,
          "pb_dropped_ir_hold": _pbir_dropped_start, "pb_dropped_ir_viol": _pbir_dropped_start}

CASES = {}
for _base in ("lab0_1c10p_exhaustive", "lab0_1c10p_exhaustive_ir", "lab0_2c10p_exhaustive", "lab0_2c10p_exhaustive_ir"):
    CASES[_base.replace("_exhaustive", "") + "_hold"] = (_base, _lab0_hold, "hold")
    CASES[_base.replace("_exhaustive", "") + "_viol"] = (_base, _lab0_viol, "viol")
CASES.update({
    "prio_inv": ("lab0_1c10p_exhaustive_ir", _prio_inv, "viol"),
    "prio_goal": ("lab0_1c10p_exhaustive_ir", _prio_goal, "viol"),
    "kv_test09_ir_hold": ("kv_test09_ir", _kv_hold, "hold"),
    "kv_test09_ir_viol": ("kv_test09_ir", _kv_viol, "viol"),
    "sipaxos_2p3a_d6_hold": ("sipaxos_2p3a_d6", _sip_hold, "hold"),
    "sipaxos_2p3a_d6_viol": ("sipaxos_2p3a_d6", _sip_viol, "viol"),
    "synth_c3_d3_hold": ("synth_c3_d3", _synth_hold, "hold"),
    "synth_c3_d3_viol": ("synth_c3_d3", _synth_viol, "viol"),
    "minitest_viol": ("minitest", _mini, "viol"),
    "mp_c5_d8_hold": ("mp_c5_d8", _mp_hold, "hold"),
    "mp_c5_d8_slotout": ("mp_c5_d8", _mp_slotout_viol, "viol"),
    "mp_c5_d8_ir_hold": ("mp_c5_d8_ir", _mp_hold, "hold"),
    "mp_c5_d8_ir_slotout": ("mp_c5_d8_ir", _mp_slotout_viol, "viol"),
    "mp_c5_d8_ir_eight": ("mp_c5_d8_ir", _mp_eight, "viol"),
    "mp_c5_d8_ir_fires": ("mp_c5_d8_ir", _mp_fires, "viol"),
    "mp_c5_d8_ir_heard": ("mp_c5_d8_ir", _mp_heard, "viol"),
    "mp_c5_d8_ir_active": ("mp_c5_d8_ir", _mp_active, "viol"),
    "mp_c5_d8_done": ("mp_c5_d8", _mp_done, "viol"),
    "pb_2s1c_d7_ir_hold": ("pb_2s1c_d7_ir", _pb_hold, "hold"),
    "pb_2s1c_d7_ir_viol": ("pb_2s1c_d7_ir", _pb_viol, "viol"),
    "pb_stage2_hold": ("pb_stage2", _pb2_hold, "hold"),
    "pb_stage2_viol": ("pb_stage2", _pb2_viol, "viol"),
    "pb_dropped_hold": ("pb_stage2", _pbd_hold, "hold"),
    "pb_dropped_viol": ("pb_stage2", _pbd_viol, "viol"),
    "pb_dropped_ir_hold": ("pb_2s1c_d7_ir", _pbd_hold, "hold"),
    "pb_dropped_ir_viol": ("pb_2s1c_d7_ir", _pbd_viol, "viol"),
})


def gold(name=None):
    with open(GOLDEN) as f:
        g = json.load(f)
    return g if name is None else g[name]


def case(name, steps=True, rows=None):
    """(protocol, settings, start state or None); steps=False: the same search without its step
    invariants (a priority case keeps its state invariant or goal). rows: the fixture generator's
    rows so far (a start taken from another case's answer; default: the committed file's)."""
    base, build, _ = CASES[name]
    proto, s, state = event_cases.case(base)
    if name in STARTS:
        state = STARTS[name](proto, rows)
    build(proto, s)
    if not steps:
        s.clearStepInvariants()
    return proto, s, state


def blob(proto, settings, state=None):
    """What stepcheck reads: watch_cases.blob, then the step invariants as dsl_set_step_invariants
    takes them (n, n_pool, 8 + 48 dsl_predicate)."""
    st = state if state is not None else proto.initial_state()
    _, w, n, pool, n_pool = settings._encode_steps(st)
    w = w if w is not None else (_lib.dsl_predicate * _lib.DSL_MAX_STEP_INVARIANTS)()
    pool = pool if pool is not None else (_lib.dsl_predicate * _lib.DSL_MAX_POOL)()
    i32 = lambda v: int(v).to_bytes(4, "little", signed=True)  # noqa: E731
    return watch_cases.blob(proto, settings, state) + i32(n) + i32(n_pool) + bytes(w) + bytes(pool)


def stepcheck_build(kind="plain"):
    out = os.path.join(HERE, "hostcheck", "_build", "stepcheck_" + kind)
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


def stepcheck_run(exe, name, tmp_dir=None, rows=None, start=None):
    """start: another start state for the case's search (default: the case's own)."""
    proto, settings, state = case(name, rows=rows)
    state = start if start is not None else state
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
