"""Multi-Paxos with a mutant (adopt-chosen-only, accept-stale) on the MI355X engine: the
searches that END with a log invariant false, against the oracle's fixtures (tests/golden/
multipaxos.json mp_mut*, watch.json mp_mut1_watch_logs; the oracle evaluates every predicate in
full on every state). What they pin is the verdict "violated" of slot_valid, logs_consistent and its
incremental form in k_level, appends_linearizable, the slotValid leaf and the generated predicates:
the level that ends the search, every terminal of it, the reported predicate and its index, and a
trace that the oracle replays into a state where that invariant is false -- on the hand-written
protocol and the one generated from the IR, in every launch mode, sharded, with sleep sets on and off."""
import json
import os

import pytest

import argmap
import oracle_util
import watch_cases
from dslabs_amd import EndCondition, Engine
from test_ir import _mp_ir, _mp_oracle_args

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "multipaxos.json")) as _f:
    GOLD = json.load(_f)

FORMS = ["MultiPaxos", "MultiPaxosIR"]
LOGS = ["mp_mut1_logs", "mp_mut2_logs", "mp_mut1_logs_active"]
SLOTVALID = ["mp_mut1_slotvalid", "mp_mut2_slotvalid"]
MODES = [{}, {"DSL_NO_QUEUE": "1"}, {"DSL_QUEUE_ROWS": "64"}]  # queued levels, one launch per level, queues that spill
_MODE_KEYS = ("DSL_NO_QUEUE", "DSL_QUEUE_ROWS")


def _setup(name, form):
    """(fixture, protocol, its settings, the oracle's arguments for a replay)"""
    case = GOLD[name]
    args = [a for a in case["args"] if a != "--finish-level"]
    if form == "MultiPaxos":
        proto = argmap.protocol(args)
        return case, proto, argmap.settings(args, proto, table_log2=22), args
    proto, rest = _mp_ir(args)
    return case, proto, argmap.settings(rest, proto, table_log2=22), _mp_oracle_args(proto, rest)


def _bfs(proto, settings, **eng):
    e = Engine(proto, **eng)
    try:
        return e.bfs(proto.initial_state(), settings)
    finally:
        e.close()


def _set_mode(monkeypatch, mode):
    for k in _MODE_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in mode.items():
        monkeypatch.setenv(k, v)


def _check_search(r, case, settings):
    """The search is the fixture's: its end, every level, the violation's depth, the predicate."""
    assert r.endCondition().name == case["end"] == "INVARIANT_VIOLATED"
    assert r.per_depth == case["per_depth"]
    assert r.states == case["states"]
    assert r.max_depth == case["terminal_depth"]
    p = r.invariantViolated()
    assert p is not None and p.value is False
    assert p.predicate is settings.invariants()[case["predicate_index"]]
    assert p.predicate.name == case["predicate"]
    assert r.invariantViolatingState().depth() == case["terminal_depth"]


def _check_replay(state, case, oargs):
    """The oracle steps through the trace and finds the fixture's invariant false at its end."""
    rep = oracle_util.replay(oargs, state.trace())
    assert rep["ok"], rep["error"]
    assert rep["depth"] == state.depth() == case["terminal_depth"]
    inv = rep["invariants"][case["predicate_index"]]
    assert inv["value"] is False and not inv["threw"], rep["invariants"]
    assert all(x["value"] for x in rep["invariants"][:case["predicate_index"]])  # the first false one is reported


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", LOGS + SLOTVALID)
def test_parity_and_trace(name, form):
    case, proto, s, oargs = _setup(name, form)
    r = _bfs(proto, s)
    print(name, form, r.per_depth, r.invariantViolated().predicate.name)
    _check_search(r, case, s)
    _check_replay(r.invariantViolatingState(), case, oargs)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", LOGS + SLOTVALID)
def test_launch_modes(name, form, monkeypatch):
    """One launch per level and queues of 64 rows (which spill) find what the queued levels find."""
    case, proto, s, _ = _setup(name, form)
    for mode in MODES[1:]:  # {} is test_parity_and_trace
        _set_mode(monkeypatch, mode)
        _check_search(_bfs(proto, s), case, s)


@pytest.mark.parametrize("rep", [0, 2000])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", LOGS + SLOTVALID)
def test_sharded(name, form, rep):
    """8 virtual shards, every level routed (replicate_below 0) or the small ones replicated."""
    case, proto, s, oargs = _setup(name, form)
    r = _bfs(proto, s, virtual_shards=8, replicate_below=rep)
    _check_search(r, case, s)
    if rep == 0:
        _check_replay(r.invariantViolatingState(), case, oargs)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", SLOTVALID)
def test_all_terminals(name, form, monkeypatch):
    """Every terminal of the violating level (the oracle finds 4): each one's trace ends, on the
    oracle, in a state with slotValid:1 false; the launch modes list the same set of states."""
    case, proto, s, oargs = _setup(name, form)
    s.maxTerminals(16)
    sets = []
    for mode in MODES:
        _set_mode(monkeypatch, mode)
        r = _bfs(proto, s)
        _check_search(r, case, s)
        assert r.numTerminals() == case["num_terminals"] == 4
        ts = r.terminals()
        assert len(ts) == 4 and len({t.packed for _, _, t in ts}) == 4
        for end, p, t in ts:
            assert end == EndCondition.INVARIANT_VIOLATED
            assert p.predicate is s.invariants()[3] and p.predicate.name == "Logs consistent for slot 1"
            if not mode:
                _check_replay(t, case, oargs)
        sets.append({t.packed for _, _, t in ts})
    assert sets[0] == sets[1] == sets[2]


@pytest.mark.parametrize("form", FORMS)
def test_appends_not_linearizable(form):
    """mp_mut1_appends: APPENDS_LINEARIZABLE alone, first false at depth 12 (483,782 states)."""
    case, proto, s, oargs = _setup("mp_mut1_appends", form)
    r = _bfs(proto, s)
    _check_search(r, case, s)
    _check_replay(r.invariantViolatingState(), case, oargs)


@pytest.mark.parametrize("form", FORMS)
def test_watched_log_predicates(form):
    """mp_mut1_watch_logs: no invariant ends the search, so it passes the first violation (depth 8, a
    slot chosen without a majority) and reaches servers with different chosen commands (depth 10,
    slot_valid's conflict branch); the four negated predicates per depth are the oracle's counts."""
    from dslabs_amd import protocols
    gold = watch_cases.gold("mp_mut1_watch_logs")
    proto, s, _ = watch_cases.mut1_watch_logs(getattr(protocols, form))
    r = _bfs(proto, s)
    c = r.watchCounts()
    print(form, c)
    assert r.endCondition().name == "SPACE_EXHAUSTED" and r.per_depth == gold["per_depth"]
    assert len(c) == 4 and c == gold["census"]
    assert sum(gold["chosen_conflict"]) > 0 and r.watchFirstDepth(0) == 8


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", LOGS + SLOTVALID)
def test_sleep_sets_on_against_off(name, form, monkeypatch):
    """The mutants deliver events the protocol's no-op filter skips (a stale P2a): the sleep-set
    rule must not lose a state of theirs either."""
    case, proto, s, _ = _setup(name, form)
    got = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("DSL_NO_SLEEP", "1")
        else:
            monkeypatch.delenv("DSL_NO_SLEEP", raising=False)
        r = _bfs(proto, s)
        _check_search(r, case, s)
        got.append((r.per_depth, r.states, r.successors, r.max_depth, r.invariantViolatingState().depth()))
    assert got[0] == got[1]
