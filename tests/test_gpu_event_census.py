"""The event census on the engine (SearchSettings.eventCensus -> k_event_census): every case of
tests/event_cases.py gives, cell for cell, the rows tests/hostcheck/eventcheck.cpp computed on the
host with exact state equality (tests/golden/event_census.json); the census changes nothing else
of a search; it is independent of table growth and restarts, of do_checks and of a time limit (a
prefix); it follows a staged start; it is refused on several shards before any collective; and a
DFS or a replay reports no rows."""
import ctypes

import pytest

import argmap
import event_cases
from dslabs_amd import CLIENTS_DONE, EndCondition, Engine, SearchSettings, _lib
from dslabs_amd.protocols import MultiPaxos

pytestmark = pytest.mark.gpu
NAMES = sorted(event_cases.CASES)


def gold_rows(name):
    g = event_cases.gold(name)
    return [event_cases.dense(r, g["classes"], g["nodes"]) for r in g["rows"]]


def _bfs(proto, settings, state=None, engine=None):
    e = engine or Engine(proto)
    try:
        return e.bfs(state if state is not None else proto.initial_state(), settings)
    finally:
        if engine is None:
            e.close()


def _check(r, name, whole=True):
    g = event_cases.gold(name)
    assert r.per_depth == g["per_depth"] and r.initial_depth == g["initial_depth"]
    assert r.eventRows() == gold_rows(name)
    if whole:
        assert r.successors == g["successors"]
    event_cases.check_identities(r.eventRows(), r.per_depth, r.successors, whole)


# ---- 1. every case against the host's rows --------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in NAMES if n != "pb_stage2"])
def test_rows_equal_the_host_walk(name):
    proto, s, state = event_cases.case(name)
    r = _bfs(proto, s.eventCensus(), state)
    _check(r, name)
    g = event_cases.gold(name)
    assert (r.endCondition() == EndCondition.SPACE_EXHAUSTED) == (g["end"] == 0)
    # the dict forms: the cells with events, by name, and their sum
    cls, adr = [n for n, _ in proto.event_classes()], proto.addresses
    cen = r.eventCensus()
    assert len(cen) == len(g["rows"])
    for d, cells in zip(cen, g["rows"]):
        assert {k: tuple(v) for k, v in d.items()} == {(cls[c], adr[t]): tuple(v) for c, t, *v in cells}
    tot = r.eventTotals()
    assert sum(v.events for v in tot.values()) == r.successors
    assert all(v.revisits == v.events - v.noops - v.exceptions - v.fresh >= 0 for v in tot.values())
    for cname, addr in event_cases.ZERO_CELLS.get(name, []):
        assert (cname, addr) not in tot


# ---- 2. the census changes nothing else ---------------------------------------------------------------------------
def same_state_and_a_trace_to_it(engine, start, x, y, replay=True):
    """x and y are the same state at the same depth, each with a trace that leads to it. The traces
    themselves may differ: a state with several parents is traced through whichever reached it
    first (include/dslabs_hip.h: "a state with two parents may be traced through either"), and the
    census runs the levels one by one instead of queued on the device, which changes who is first.
    So each trace is replayed on the host and must end in the state (not an exceptional one's: its
    last event throws)."""
    assert x.packed == y.packed and x.depth() == y.depth() and len(x.trace()) == len(y.trace())
    for st in (x, y):
        if st.packed is None or not replay:
            continue
        rp = engine.replay(start if start is not None else st.protocol.initial_state(), SearchSettings(), st.events(),
                           minimize=False)
        last = rp.lastState()
        assert last is not None and last.packed == st.packed and last.depth() == st.depth()


@pytest.mark.parametrize("name", ["mp_c5_d8", "pb_initview", "minitest", "lab0_2c3p_notimers"])
def test_search_is_the_same_with_and_without(name):
    proto, s, state = event_cases.case(name)
    s.maxTerminals(8).addWatch(proto.raw_field(0, 0, 1) == 0, witness=True)  # a generic leaf: every protocol takes it
    e = Engine(proto)
    try:
        a = _bfs(proto, s, state, e)
        b = _bfs(proto, s.clone().eventCensus(), state, e)
        c = _bfs(proto, s, state, e)  # and off again on the same engine
        assert a.eventRows() == [] and c.eventRows() == [] and b.eventRows() == gold_rows(name)
        for r in (b, c):
            assert (r.states, r.per_depth, r.successors) == (a.states, a.per_depth, a.successors)
            assert r.endCondition() == a.endCondition()
            assert r.numTerminals() == a.numTerminals() and len(r.terminals()) == len(a.terminals())
            for (e1, p1, s1), (e2, p2, s2) in zip(r.terminals(), a.terminals()):
                assert e1 == e2 and (p1 is None) == (p2 is None)
                same_state_and_a_trace_to_it(e, state, s1, s2, e1 != EndCondition.EXCEPTION_THROWN)
            ta, tr = a.lastState(), r.lastState()
            assert (ta is None) == (tr is None)
            if ta is not None:
                same_state_and_a_trace_to_it(e, state, tr, ta, a.endCondition() != EndCondition.EXCEPTION_THROWN)
            assert r.watchCounts() == a.watchCounts() and r.watchTotal(0) == a.watchTotal(0)
            wa, wr = a.watchWitness(0), r.watchWitness(0)
            assert (wa is None) == (wr is None)
            if wa is not None:
                same_state_and_a_trace_to_it(e, state, wr, wa)
    finally:
        e.close()


# ---- 3. table growth and a restart, do_checks -----------------------------------------------------------------------
def test_small_first_table_grows_and_restarts_with_the_same_rows():
    proto, s, _ = event_cases.case("mp_c5_d8")
    s.table_log2_slots = 10
    e = Engine(proto)
    try:
        r = e.bfs(proto.initial_state(), s.eventCensus())
        st = e.kernel_stats()
    finally:
        e.close()
    assert st["table_slots"] > (1 << 10) or st["table_rehashes"] > 0  # it grew
    _check(r, "mp_c5_d8")


def test_do_error_checks_gives_the_same_rows():
    proto, s, _ = event_cases.case("mp_c5_d8")
    r = _bfs(proto, s.eventCensus().doErrorChecks())
    assert r.checks["run"] > 0 and r.checks["not_deterministic"] == 0
    _check(r, "mp_c5_d8")


# ---- 4. a time limit: a prefix ---------------------------------------------------------------------------------------
def test_time_limited_rows_are_a_prefix():
    proto = MultiPaxos(3, 2, "append-xy")
    args = event_cases.CASES["mp_c5_d8"][0]
    k = args.index("--max-depth")
    deep = argmap.settings(args[:k] + ["--max-depth", "12"] + args[k + 2:], proto, table_log2=24).eventCensus()
    e = Engine(proto)
    try:
        full = e.bfs(proto.initial_state(), deep)  # the warm-up, and the unlimited rows
        assert full.endCondition() == EndCondition.SPACE_EXHAUSTED and len(full.eventRows()) == 12
        assert full.eventRows()[:8] == gold_rows("mp_c5_d8")
        event_cases.check_identities(full.eventRows(), full.per_depth, full.successors)
        r = e.bfs(proto.initial_state(), deep.clone().maxTimeSecs(0.001))  # 1 ms: the twelve levels with the census take about three
    finally:
        e.close()
    rows = r.eventRows()
    print("time-limited:", r.endCondition().name, "rows", len(rows), "per_depth", len(r.per_depth))
    assert len(rows) <= 12 - r.initial_depth and rows == full.eventRows()[:len(rows)]
    assert r.per_depth == full.per_depth[:len(r.per_depth)]
    # one row per completed level: every depth of per_depth but the last was expanded completely
    assert len(rows) == len(r.per_depth) - 1 or r.endCondition() == EndCondition.SPACE_EXHAUSTED
    event_cases.check_identities(rows, r.per_depth, r.successors, r.endCondition() == EndCondition.SPACE_EXHAUSTED)


# ---- 5. a second stage from the first stage's goal state ----------------------------------------------------------------
def test_second_stage_from_the_first_stages_goal_state():
    proto, s1, _ = event_cases.case("pb_initview")
    e = Engine(proto)
    try:
        r1 = e.bfs(proto.initial_state(), s1.eventCensus())
        goal = r1.goalMatchingState()
        want = event_cases.gold("pb_initview")["terminal"]
        # the host walk's terminal is the engine's: the fixture's second stage starts where this one does
        assert goal is not None and goal.depth() == want["depth"] and goal.packed.hex() == want["state"]
        _, s2, _ = event_cases.case("pb_stage2")
        st = event_cases.stage2_start(proto, goal.packed.hex(), goal.depth())
        assert st.droppedMessages() and st.depth() == 11
        r2 = e.bfs(st, s2.eventCensus())
    finally:
        e.close()
    _check(r1, "pb_initview")
    _check(r2, "pb_stage2")
    assert r2.initial_depth == 11 and len(r2.eventRows()) == 5


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_census_is_refused_on_several_shards():
    proto, s, _ = event_cases.case("mp_c5_d8")
    e = Engine(proto, virtual_shards=3, replicate_below=0)
    try:
        with pytest.raises(_lib.EngineError) as err:
            e.bfs(proto.initial_state(), s.clone().eventCensus())
        assert err.value.code == -1 and "dsl_run" in str(err.value)
        assert "event census is not supported in a search over more than one shard" in str(err.value)
        r = e.bfs(proto.initial_state(), s)  # the same engine, with the census off
        assert r.per_depth == event_cases.gold("mp_c5_d8")["per_depth"] and r.eventRows() == []
    finally:
        e.close()


def test_a_search_over_several_processes_refuses_the_census_before_any_collective():
    from dslabs_amd import distributed as d
    from dslabs_amd.protocols import PingPong
    calls = []

    def cb(*_):
        calls.append(1)
        return 1

    class Comm:
        cbs = (d.ALLGATHER(cb), d.ALLREDUCE(cb), d.BCAST(cb), d.ALLTOALLV(cb))
        struct = d.dsl_host_comm(None, 0, 2, *cbs, 0, 0)

    proto = PingPong(1, 2)
    e = Engine(proto, rank=0, world_size=2, host_comm=Comm())
    try:
        with pytest.raises(_lib.EngineError) as err:
            e.bfs(proto.initial_state(), SearchSettings().eventCensus())
        assert err.value.code == -1 and "event census" in str(err.value)
        assert calls == []
    finally:
        e.close()


def test_dfs_and_replay_report_no_rows_and_c_abi_bounds():
    proto, s, _ = event_cases.case("lab0_1c10p_exhaustive_ir")
    goal = SearchSettings().addGoal(CLIENTS_DONE).eventCensus()
    goal.table_log2_slots = 20
    e = Engine(proto)
    try:
        n = ctypes.c_int32(-1)
        assert e.lib.dsl_event_census(e.handle, 0, None, ctypes.byref(n)) == 0 and n.value == 0  # before any search
        r = e.bfs(proto.initial_state(), s.eventCensus())
        _check(r, "lab0_1c10p_exhaustive_ir")
        assert e.lib.dsl_event_census(e.handle, 0, None, ctypes.byref(n)) == 0 and n.value == 29
        cells = (_lib.dsl_event_count * (_lib.DSL_EVENT_CLASSES * _lib.DSL_EVENT_NODES))()
        for bad in (-1, 29, 1 << 20):
            assert e.lib.dsl_event_census(e.handle, bad, cells, None) == -1
            assert b"dsl_event_census: level" in e.lib.dsl_last_error()
        assert e.lib.dsl_event_census(e.handle, 28, cells, None) == 0
        # cells outside the protocol's classes and nodes are zero
        ncls, nn = len(proto.event_classes()), len(proto.addresses)
        for c in range(_lib.DSL_EVENT_CLASSES):
            for t in range(_lib.DSL_EVENT_NODES):
                x = cells[c * _lib.DSL_EVENT_NODES + t]
                if c >= ncls or t >= nn:
                    assert (x.events, x.noops, x.exceptions, x.fresh) == (0, 0, 0, 0)
        g = e.bfs(proto.initial_state(), goal)
        assert g.endCondition() == EndCondition.GOAL_FOUND and len(g.eventRows()) == 20  # the goal's level is a row
        d = e.dfs(proto.initial_state(), goal.clone().maxDepth(30), probes=256, max_probes=256, seed=1)  # one launch
        assert d.eventRows() == [] and d.eventCensus() == [] and d.eventTotals() == {}
        assert e.lib.dsl_event_census(e.handle, 0, None, ctypes.byref(n)) == 0 and n.value == 0
        assert e.bfs(proto.initial_state(), goal).eventRows() == g.eventRows()
        rp = e.replay(proto.initial_state(), goal, g.goalMatchingState().events())
        assert rp.endCondition() == EndCondition.GOAL_FOUND and rp.eventRows() == []
        assert e.lib.dsl_event_census(e.handle, 0, None, ctypes.byref(n)) == 0 and n.value == 0
        # a search without the census on an engine that never had it makes no new C call
        e2 = Engine(proto)
        try:
            plain = e2.bfs(proto.initial_state(), s.clone().eventCensus(False))
            assert plain.eventRows() == [] and not hasattr(e2, "_set_event_census")
        finally:
            e2.close()
    finally:
        e.close()
