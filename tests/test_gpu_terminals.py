"""Every terminal state of the level that ends a BFS (SearchSettings.maxTerminals): the set, the
order, the cap and the traces against the CPU oracle's --finish-level list (Search.java:370-385,
:468-504). The list never depends on arrival order, on DSL_TERM_CAP or on sharding, and its first
entry is the terminal the search reports."""
import collections
import json
import os
import re

import pytest

import argmap
import oracle_util
from dslabs_amd import Engine, EndCondition, SearchSettings, _lib
from test_gpu_terminal import CASES as TERM_CASES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LIST = ["--finish-level", "--print-states", "--max-terminals", "100000"]
SHARDED = {"virtual_shards": 3, "replicate_below": 0}


def _golden(fname, name):
    with open(os.path.join(HERE, "golden", fname)) as f:
        return [a for a in json.load(f)[name]["args"] if a != "--finish-level"]


def _plain(args):
    """A hand-written protocol: the oracle takes the fixture's arguments as they are."""
    proto = argmap.protocol(args)
    return proto, args, args


def _mp_ir(args):
    from test_ir import _mp_ir, _mp_oracle_args
    proto, rest = _mp_ir(args)
    return proto, rest, _mp_oracle_args(proto, rest)


def _pb_ir(args):
    from test_ir import _pb_ir, _pb_oracle_args
    proto, rest = _pb_ir(args)
    return proto, rest, _pb_oracle_args(proto, rest)


# name -> (protocol, the arguments argmap.settings reads, the oracle's arguments)
ROWS = {
    "kv_appendappendget_2c": lambda: _plain(_golden("amokv.json", "kv_appendappendget_2c")),
    "kv_getput_2c": lambda: _plain(_golden("amokv.json", "kv_getput_2c")),
    "mp_expect_violation": lambda: _plain(_golden("multipaxos.json", "mp_expect_violation")),
    "mp_expect_violation_ir": lambda: _mp_ir(_golden("multipaxos.json", "mp_expect_violation")),
    "pb_view3_goal": lambda: _plain(_golden("pb.json", "pb_view3_goal")),
    "pb_view3_goal_ir": lambda: _pb_ir(_golden("pb.json", "pb_view3_goal")),  # a network predicate
    "pb_2c_results_violation": lambda: _plain(_golden("pb.json", "pb_2c_results_violation")),
    "synth_counter_violation": lambda: _plain(_golden("synthetic.json", "synth_counter_violation")),
    "synth_3n_k8_d9": lambda: _plain(_golden("synthetic.json", "synth_3n_k8_d9")),
    "minitest_exception_and_invariant": lambda: _plain(["--proto", "minitest", "--inv", "foo"]),
    "invariant_beats_goals": lambda: _plain(TERM_CASES["invariant_beats_goals"]),
    "many_goals_one_invariant": lambda: _plain(TERM_CASES["many_goals_one_invariant"]),
}
# terminals of the final level, by kind (the issue's table, from the CPU oracle)
KINDS = {
    "kv_appendappendget_2c": {"INVARIANT_VIOLATED": 2}, "kv_getput_2c": {"INVARIANT_VIOLATED": 2},
    "mp_expect_violation": {"INVARIANT_VIOLATED": 2}, "mp_expect_violation_ir": {"INVARIANT_VIOLATED": 2},
    "pb_view3_goal": {"GOAL_FOUND": 6}, "pb_view3_goal_ir": {"GOAL_FOUND": 6},
    "pb_2c_results_violation": {"INVARIANT_VIOLATED": 4},
    "synth_counter_violation": {"INVARIANT_VIOLATED": 7}, "synth_3n_k8_d9": {"INVARIANT_VIOLATED": 8},
    "minitest_exception_and_invariant": {"EXCEPTION_THROWN": 1, "INVARIANT_VIOLATED": 1},
    "invariant_beats_goals": {"INVARIANT_VIOLATED": 12, "GOAL_FOUND": 60},
    "many_goals_one_invariant": {"INVARIANT_VIOLATED": 116, "GOAL_FOUND": 2204},
}
_cache = {}


def _case(name):
    """(protocol, settings arguments, oracle arguments, the oracle's finished level), computed once."""
    if name not in _cache:
        proto, sargs, oargs = ROWS[name]()
        _cache[name] = (proto, sargs, oargs, oracle_util.run("bfs", oargs + LIST, timeout=300))
    return _cache[name]


def _key(state):
    """An oracle state key without the identity counter of an exceptional state."""
    return re.sub(r"EXC#\d+$", "", state)


def _search(name, max_terminals, engine=None, **eng):
    proto, sargs, _, _ = _case(name)
    s = argmap.settings(sargs, proto, table_log2=22)
    if max_terminals is not None:
        s.maxTerminals(max_terminals)
    e = engine or Engine(proto, **eng)
    try:
        return e.bfs(proto.initial_state(), s), s
    finally:
        if engine is None:
            e.close()


def _triples(r):
    return [(end, None if p is None else p.predicate.name, st.packed) for end, p, st in r.terminals()]


def _check_entry(name, settings, entry, rep):
    """The replayed state is a terminal of the entry's kind and predicate index: the first invariant
    that is false or threw, or (every invariant holding) the first goal that is true."""
    end, pred, st = entry
    assert rep["ok"], rep["error"]
    assert rep["depth"] == st.depth() and len(st.trace()) == len(st.events())
    bad = [i for i, x in enumerate(rep["invariants"]) if x["threw"] or not x["value"]]
    if end == EndCondition.EXCEPTION_THROWN:
        assert rep["exception"] and pred is None
        return
    assert not rep["exception"]
    if end == EndCondition.INVARIANT_VIOLATED:
        assert pred.value is False and bad and settings.invariants()[bad[0]] is pred.predicate
    else:
        assert end == EndCondition.GOAL_FOUND and not bad
        hit = [i for i, x in enumerate(rep["goals"]) if x["value"]]
        assert pred.value is True and hit and settings.goals()[hit[0]] is pred.predicate


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("name", sorted(n for n in ROWS if n != "many_goals_one_invariant"))
def test_terminal_set_equals_the_oracles(name, shards):
    _, _, oargs, want = _case(name)
    assert dict(collections.Counter(t["kind"] for t in want["terminals"])) == KINDS[name]
    r, s = _search(name, 4096, **(SHARDED if shards > 1 else {}))
    _check_set(name, r, s, oargs, want)


def test_terminal_level_is_the_first_sharded_level(monkeypatch, capfd):
    """The listing pass with the owner filter on: the levels below the terminal level's frontier
    (66 Multi-Paxos parents, six chunks of at most 12) run replicated, so the terminal level is the
    first sharded one -- every shard holds all its parents and expands only those it owns, and the
    pass must skip the others (parents of no work item between parents that have some)."""
    name = "mp_expect_violation"
    _, _, oargs, want = _case(name)
    monkeypatch.setenv("DSL_LEVEL_TRACE", "1")
    r, s = _search(name, 4096, virtual_shards=3, replicate_below=want["per_depth"][-2])
    sharded = re.findall(r"^\[level\] .* sharded=(\d)", capfd.readouterr().err, re.M)
    assert len(sharded) > 1 and sharded == ["0"] * (len(sharded) - 1) + ["1"]
    _check_set(name, r, s, oargs, want)


def _check_set(name, r, s, oargs, want):
    assert r.endCondition().name == want["end"]
    assert r.per_depth == want["per_depth"]
    assert r.numTerminals() == want["num_terminals"] == len(r.terminals())
    assert dict(collections.Counter(end.name for end, _, _ in r.terminals())) == KINDS[name]
    assert (len(r.exceptionalStates()), len(r.invariantViolatingStates()), len(r.goalMatchingStates())) == tuple(
        KINDS[name].get(k, 0) for k in ("EXCEPTION_THROWN", "INVARIANT_VIOLATED", "GOAL_FOUND"))
    keys = []
    for entry in r.terminals():
        rep = oracle_util.replay(oargs, entry[2].trace())
        _check_entry(name, s, entry, rep)
        keys.append(_key(rep["state"]))
    assert len(set(keys)) == len(keys)  # each state once
    assert set(keys) == {_key(t["state"]) for t in want["terminals"]}
    # the first entry is the terminal the search reports
    first = r.terminals()[0]
    reported = r.exceptionalState() or r.invariantViolatingState() or r.goalMatchingState()
    assert first[0] == r.endCondition() and first[2].packed == reported.packed


def test_order_cap_and_determinism(monkeypatch):
    name = "invariant_beats_goals"
    monkeypatch.delenv("DSL_TERM_CAP", raising=False)
    r, _ = _search(name, 4096)
    full = _triples(r)
    assert [t[0] for t in full] == [EndCondition.INVARIANT_VIOLATED] * 12 + [EndCondition.GOAL_FOUND] * 60
    assert r.terminals()[0][2].packed == r.invariantViolatingState().packed
    assert r.terminals()[0][1].predicate is r.invariantViolated().predicate
    capped, _ = _search(name, 10)
    assert capped.numTerminals() == 72 and _triples(capped) == full[:10]
    # the same list whatever the arrival order, the reported terminal's resolution or the sharding
    monkeypatch.setenv("DSL_TERM_CAP", "0")
    assert _triples(_search(name, 4096)[0]) == full
    monkeypatch.delenv("DSL_TERM_CAP")
    assert _triples(_search(name, 4096, **SHARDED)[0]) == full
    assert _triples(_search(name, 4096, virtual_shards=3)[0]) == full  # the default replication rule
    proto = _case(name)[0]
    e = Engine(proto)
    try:
        assert _triples(_search(name, 4096, engine=e)[0]) == full
        assert _triples(_search(name, 4096, engine=e)[0]) == full  # a second run on the same engine
    finally:
        e.close()


@pytest.mark.parametrize("shards", [1, 3])
def test_level_larger_than_any_default_list(shards):
    name = "many_goals_one_invariant"
    _, _, oargs, want = _case(name)
    assert want["num_terminals"] == 2320
    assert dict(collections.Counter(t["kind"] for t in want["terminals"])) == KINDS[name]
    r, s = _search(name, 4096, **(SHARDED if shards > 1 else {}))
    assert r.endCondition().name == want["end"] and r.per_depth == want["per_depth"]
    ts = r.terminals()
    assert r.numTerminals() == 2320 == len(ts)
    assert len({st.packed for _, _, st in ts}) == 2320
    assert [end for end, _, _ in ts] == [EndCondition.INVARIANT_VIOLATED] * 116 + [EndCondition.GOAL_FOUND] * 2204
    assert ts[0][2].packed == r.invariantViolatingState().packed
    want_keys = {_key(t["state"]) for t in want["terminals"]}
    picks = sorted({0, len(ts) - 1} | set(range(37, len(ts), 75)[:30]))
    assert len(picks) == 32
    for i in picks:
        rep = oracle_util.replay(oargs, ts[i][2].trace())
        _check_entry(name, s, ts[i], rep)
        assert _key(rep["state"]) in want_keys


def test_off_by_default_and_empty_without_a_terminal():
    # max_terminals 0: no list, and the result is the one a search without the setting gives
    base, _ = _search_goals_only(None)
    off, _ = _search_goals_only(0)
    on, _ = _search_goals_only(4096)
    for r in (base, off):
        assert r.terminals() == [] and r.numTerminals() == 0 and r.goalMatchingStates() == []
    for r in (off, on):
        assert r.endCondition() == base.endCondition() == EndCondition.GOAL_FOUND
        assert (r.per_depth, r.states, r.max_depth, r.successors) == (base.per_depth, base.states, base.max_depth,
                                                                     base.successors)
        assert r.goalMatchingState().packed == base.goalMatchingState().packed
        assert r.goalMatched().predicate.name == base.goalMatched().predicate.name
    assert on.numTerminals() == 72 and on.terminals()[0][2].packed == base.goalMatchingState().packed
    # a search that ends without a terminal lists nothing
    with open(os.path.join(HERE, "golden", "lab0.json")) as f:
        case = json.load(f)["lab0_1c2p_exhaustive"]
    proto = argmap.protocol(case["args"])
    e = Engine(proto)
    try:
        r = e.bfs(proto.initial_state(), argmap.settings(case["args"], proto, table_log2=22).maxTerminals(8))
    finally:
        e.close()
    assert r.endCondition() == EndCondition.SPACE_EXHAUSTED
    assert r.per_depth == case["per_depth"]
    assert r.terminals() == [] and r.numTerminals() == 0


def test_a_search_over_several_processes_refuses_the_list_before_any_collective():
    """world_size 2 with max_terminals > 0: DSL_ERR_ARG at the start of dsl_run, no collective called
    (every rank carries the same settings and refuses alike, so none waits for a peer)."""
    from dslabs_amd import distributed as d
    calls = []

    def cb(*_):
        calls.append(1)
        return 1

    class Comm:
        cbs = (d.ALLGATHER(cb), d.ALLREDUCE(cb), d.BCAST(cb), d.ALLTOALLV(cb))
        struct = d.dsl_host_comm(None, 0, 2, *cbs, 0, 0)

    from dslabs_amd.protocols import PingPong
    proto = PingPong(1, 2)
    e = Engine(proto, rank=0, world_size=2, host_comm=Comm())
    try:
        with pytest.raises(_lib.EngineError) as err:
            e.bfs(proto.initial_state(), SearchSettings().maxTerminals(4))
        assert err.value.code == -1 and "max_terminals" in str(err.value) and "one process" in str(err.value)
        assert calls == []
    finally:
        e.close()


def _search_goals_only(max_terminals):
    args = TERM_CASES["goals_only"]
    proto = argmap.protocol(args)
    s = argmap.settings(args, proto, table_log2=22)
    if max_terminals is not None:
        s.maxTerminals(max_terminals)
    e = Engine(proto)
    try:
        return e.bfs(proto.initial_state(), s), s
    finally:
        e.close()
