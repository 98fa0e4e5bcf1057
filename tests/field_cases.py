"""Golden fixtures restated with user-written field predicates (FieldRef comparisons, DSL_PRED_FIELD),
shared by the CPU-baseline and the engine tests. Every expected value comes from the committed
fixture (written by the oracle with the NAMED predicates), never from the code under test."""
import json
import os

import argmap
from dslabs_amd import SearchSettings, allOf
from dslabs_amd.protocols import PingPongIR

HERE = os.path.dirname(os.path.abspath(__file__))


def gold(fname, name):
    with open(os.path.join(HERE, "golden", fname + ".json")) as f:
        return json.load(f)[name]


def client_done(proto, client, pings=10):
    """CLIENT_DONE of a repeatedPings client: all `pings` results harvested."""
    return proto.length(client, "_results") == pings


def results_ok(proto, client, pings=10):
    """RESULTS_OK of one client, as `pings` predicates: result j, when there, is Pong(j + 1)."""
    return [(proto.length(client, "_results") <= j).or_(proto.field(client, "_results", j) == j + 1)
            for j in range(pings)]


def _settings(table_log2=20):
    s = SearchSettings()
    s.table_log2_slots = table_log2
    return s


def _goal():
    p = PingPongIR(1, 10)
    return p, _settings().addGoal(client_done(p, "client1"))


def _exhaustive():
    p = PingPongIR(1, 10)
    return p, _settings().addPrune(client_done(p, "client1"))


def _exhaustive2():
    p = PingPongIR(2, 10)
    return p, _settings().addPrune(allOf([client_done(p, "client1"), client_done(p, "client2")]))


def _nocheck():
    p = PingPongIR(1, 10, check_value=False)
    s = _settings().addGoal(client_done(p, "client1"))
    for inv in results_ok(p, "client1"):
        s.addInvariant(inv)
    return p, s


def _synth(name):
    case = gold("synthetic", name)
    p = argmap.protocol(case["args"])
    v = lambda node: p.raw_field(node, 0, 16)  # noqa: E731  synthetic.hpp v_of: bits 0-15 of word 0
    if name == "synth_counter_violation":  # --inv COUNTER_LT:2:30
        return p, _settings().addInvariant(v("node3") < 30)
    # --goal !COUNTER_LT:0:63 --prune !COUNTER_LT:1:40: negated leaves
    return p, _settings().addGoal(v("node1").lt(63).negate()).addPrune(v(1).lt(40).negate())


# name -> (fixture file, builder of (protocol, settings)); the fixture's name is the case's
CASES = {
    "lab0_1c10p_goal": ("lab0", _goal),
    "lab0_1c10p_exhaustive": ("lab0", _exhaustive),
    "lab0_2c10p_exhaustive": ("lab0", _exhaustive2),
    "lab0_mutant_nocheck": ("lab0", _nocheck),
    "synth_counter_violation": ("synthetic", lambda: _synth("synth_counter_violation")),
    "synth_goal_prune": ("synthetic", lambda: _synth("synth_goal_prune")),
}


def case(name):
    fname, build = CASES[name]
    proto, settings = build()
    return gold(fname, name), proto, settings
