"""Sleep sets in k_level (dslabs_amd/csrc/nodestate.hpp) on the MI355X: the rule on
(the default) against off (DSL_NO_SLEEP, read by the engine at the start of every search). The
search must not move -- per-depth counts, states, successors, the end and its predicate, the
watches' census and witnesses, the terminal list -- while the visited-table probes fall; where the
settings forbid the rule (a prune, more than one shard) the probes stay what they were."""
import json
import os

import pytest

import argmap
import oracle_util
import witness_cases
from dslabs_amd import Engine

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _gold(fname, name):
    return json.load(open(os.path.join(HERE, "golden", fname + ".json")))[name]


def _with_depth(args, depth):
    args = list(args)
    k = args.index("--max-depth")
    return args[:k] + ["--max-depth", str(depth)] + args[k + 2:]


def _bfs(monkeypatch, sleep, proto, settings, state=None, **eng):
    if sleep:
        monkeypatch.delenv("DSL_NO_SLEEP", raising=False)
    else:
        monkeypatch.setenv("DSL_NO_SLEEP", "1")
    e = Engine(proto, **eng)
    try:
        r = e.bfs(state if state is not None else proto.initial_state(), settings)
        return r, e.kernel_stats()
    finally:
        e.close()


def _search(r):
    """What must not move: counts, the end, the terminal's depth and the predicate that fired."""
    t = r.invariantViolatingState() or r.goalMatchingState()
    p = r.invariantViolated() or r.goalMatched()
    return (r.endCondition().name, r.per_depth, r.states, r.successors, r.max_depth,
            None if t is None else t.depth(), None if p is None else (p.predicate.name, p.value))


CASES = {
    "mp_c5_d8": _gold("multipaxos", "mp_c5_d8")["args"],
    "sipaxos_d8": _with_depth(_gold("sipaxos", "sipaxos_2p3a_d9")["args"], 8),
    "mp_expect_violation": _gold("multipaxos", "mp_expect_violation")["args"],
    "mp_test27_goal": _gold("multipaxos", "mp_test27")["args"],
}
MODES = [{}, {"DSL_NO_QUEUE": "1"}, {"DSL_QUEUE_ROWS": "64"}]  # queued levels, one launch per level, tiny queues that spill


@pytest.mark.parametrize("mode", MODES, ids=lambda m: ",".join("%s=%s" % kv for kv in m.items()) or "queued")
@pytest.mark.parametrize("name", sorted(CASES))
def test_on_against_off(name, mode, monkeypatch):
    """The same search with fewer probes; its trace replays on the oracle. DSL_QUEUE_ROWS=64 makes
    the queued levels overflow their segments, so spilled rows (k_unspill: no creator) join the
    frontier."""
    for k, v in mode.items():
        monkeypatch.setenv(k, v)
    args = CASES[name]
    proto = argmap.protocol(args)
    s = argmap.settings(args, proto)
    on, st_on = _bfs(monkeypatch, True, proto, s)
    off, st_off = _bfs(monkeypatch, False, proto, s)
    print(name, mode, "probes on/off", st_on["probes"], st_off["probes"], "states", on.states)
    assert _search(on) == _search(off)
    if name == "mp_c5_d8":
        assert on.states == 17320 and on.per_depth == _gold("multipaxos", "mp_c5_d8")["per_depth"]
    t = on.invariantViolatingState() or on.goalMatchingState()
    if t is not None:
        rep = oracle_util.replay([a for a in args if a != "--finish-level"], t.trace())
        assert rep["ok"], rep["error"]
        assert rep["depth"] == t.depth()
    assert st_on["probes"] < st_off["probes"]


def test_watched_search(monkeypatch):
    """The watches' census and witnesses of C5 to depth 8 (tests/golden/watch.json, witness.json)."""
    proto, s, state = witness_cases.case("mp_c5_d8_named")
    on, st_on = _bfs(monkeypatch, True, proto, s, state)
    off, st_off = _bfs(monkeypatch, False, proto, s, state)
    n = len(on.watchCounts())
    assert _search(on) == _search(off)
    assert on.watchCounts() == off.watchCounts() == witness_cases.watch_cases.gold("mp_c5_d8_named")["census"]
    for w in range(n):
        a, b = on.watchWitness(w), off.watchWitness(w)
        assert (a is None) == (b is None)
        if a is not None:
            assert a.packed == b.packed == witness_cases.gold_state("mp_c5_d8_named", w)
            assert a.depth() == b.depth() == on.watchFirstDepth(w)
    assert st_on["probes"] < st_off["probes"]


def test_max_terminals_search(monkeypatch):
    """Every terminal of the level that ends the violation fixture: the same list, in the same order."""
    args = [a for a in _gold("multipaxos", "mp_expect_violation")["args"] if a != "--finish-level"]
    proto = argmap.protocol(args)
    s = argmap.settings(args, proto).maxTerminals(100000)
    on, st_on = _bfs(monkeypatch, True, proto, s)
    off, _ = _bfs(monkeypatch, False, proto, s)
    assert _search(on) == _search(off)
    assert on.numTerminals() == off.numTerminals() > 0
    assert [(e.name, t.packed) for e, _, t in on.terminals()] == [(e.name, t.packed) for e, _, t in off.terminals()]


def _without_prunes(args):
    out, i = [], 0
    while i < len(args):
        if args[i] == "--prune":
            i += 2
            continue
        out.append(args[i])
        i += 1
    return out


@pytest.mark.parametrize("kind", ["prune", "two_virtual_shards"])
def test_rule_stays_off(kind, monkeypatch):
    """A search with a prune (a pruned state is not expanded) and one on 2 virtual shards, both of
    Multi-Paxos, which is compiled with the rule: the probes are equal on against off. The same
    searches with the condition taken away -- no prune, one shard -- probe less with the rule on,
    so the equality is the condition's doing."""
    if kind == "prune":
        case = _gold("multipaxos", "mp_2s1c_prune")
        eng = {}
        free_args, free_eng = _without_prunes(case["args"]), {}
    else:
        # frontiers below 1,000 states run replicated -- k_level probes its own table there, and
        # dsl_stats.probes counts those probes -- and the deeper levels are routed (their probes are
        # the owners', which that counter leaves out): both kinds of level of a sharded search
        case = _gold("multipaxos", "mp_c5_d8")
        eng = {"virtual_shards": 2, "replicate_below": 1000}
        free_args, free_eng = case["args"], {}
    proto = argmap.protocol(case["args"])
    s = argmap.settings(case["args"], proto)
    on, st_on = _bfs(monkeypatch, True, proto, s, **eng)
    off, st_off = _bfs(monkeypatch, False, proto, s, **eng)
    assert _search(on) == _search(off)
    assert on.per_depth == case["per_depth"] and on.states == case["states"]
    print(kind, "probes on/off", st_on["probes"], st_off["probes"])
    assert st_on["probes"] == st_off["probes"] > 0
    free = argmap.settings(free_args, proto)
    f_on, sf_on = _bfs(monkeypatch, True, proto, free, **free_eng)
    f_off, sf_off = _bfs(monkeypatch, False, proto, free, **free_eng)
    print(kind, "without the condition: probes on/off", sf_on["probes"], sf_off["probes"])
    assert _search(f_on) == _search(f_off)
    assert sf_on["probes"] < sf_off["probes"]
