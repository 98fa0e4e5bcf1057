"""Watches (SearchSettings.addWatch) counted by the MI355X kernels: the census per watch and depth
against tests/golden/watch.json (the host truth of tests/hostcheck/watchcheck.cpp) and the oracle's
anchors, with the search itself unchanged against the oracle's fixtures; table growth and the
key-width restart, the find-mode re-run, a staged start over a dropped network, the named network
predicates, the C ABI's refusals, and searches without watches."""
import ctypes

import pytest

import watch_cases
from dslabs_amd import CLIENTS_DONE, RESULTS_OK, EndCondition, Engine, SearchSettings, StatePredicate, _lib
from dslabs_amd import search as S
from dslabs_amd.protocols import MultiPaxosIR, PingPongIR

pytestmark = pytest.mark.gpu
DSL_ERR_ARG = -1  # include/dslabs_hip.h dsl_status


def _bfs(proto, settings, state=None, **eng):
    e = Engine(proto, **eng)
    try:
        return e.bfs(state if state is not None else proto.initial_state(), settings), e.kernel_stats()
    finally:
        e.close()


def _same_search(a, b):
    return (a.endCondition(), a.states, a.per_depth, a.max_depth, a.successors) == \
        (b.endCondition(), b.states, b.per_depth, b.max_depth, b.successors)


# ---- 1. lab0: eight watches in one search -------------------------------------------------------------------
def test_pingpong_eight_watches():
    proto, s, _ = watch_cases.case("pp_1c10p_8w")
    gold, fix = watch_cases.gold("pp_1c10p_8w"), watch_cases.fixture("lab0", "lab0_1c10p_exhaustive")
    r, _ = _bfs(proto, s)
    bare, _ = _bfs(proto, s.clone().clearWatches())
    for x in (r, bare):  # the search is the fixture's, with and without the watches
        assert x.per_depth == fix["per_depth"] and x.states == fix["states"] == 120 and x.max_depth == 29
        assert x.endCondition().name == fix["end"]
    assert _same_search(r, bare) and bare.watchCounts() == []
    c = r.watchCounts()
    print("census", c)
    assert len(c) == 8 and all(len(v) == len(r.per_depth) for v in c)
    assert c == gold["census"]
    assert c[3] == r.per_depth                                        # always true
    assert [a + b for a, b in zip(c[1], c[2])] == r.per_depth          # a watch plus its negation, at every depth
    assert c[6][0] == 1 and r.watchFirstDepth(6) == 0                  # true on the start state (host-evaluated)
    assert r.watchFirstDepth(0) == 20 and c[0][20] == 1                # CLIENTS_DONE: the oracle's anchor
    assert [r.watchTotal(i) for i in range(8)] == [sum(v) for v in c] == gold["true"]


# ---- 2. mp_c5_d8: a level of many workgroups, the maxDepth level, inside the level queue --------------------
@pytest.mark.parametrize("name", ["mp_c5_d8_named", "mpir_c5_d8_named", "mpir_c5_d8_generic"])
def test_multipaxos_census(name):
    proto, s, _ = watch_cases.case(name)
    gold, fix = watch_cases.gold(name), watch_cases.fixture("multipaxos", "mp_c5_d8")
    r, _ = _bfs(proto, s)
    c = r.watchCounts()
    print(name, c)
    assert r.per_depth == fix["per_depth"] and r.states == fix["states"] == 17320
    assert r.endCondition().name == fix["end"]
    assert c == gold["census"]
    assert c[-1] == [0] * 8 + [8]  # CLIENTS_DONE (the last watch of each case)
    if name == "mpir_c5_d8_generic":
        named = watch_cases.gold("mpir_c5_d8_named")["census"]
        for k, (_, restates) in enumerate(watch_cases.MP_GENERIC):
            if restates:  # a generic restatement and the named watch give equal vectors
                assert c[k] == named[watch_cases.MP_NAMED.index(restates)], restates
        assert c[1] == c[6]  # the field leaf and the named leaf in the same search
    else:
        for (case, w), (depth, count) in watch_cases.ANCHORS.items():
            if case == "mp_c5_d8_named":  # the oracle's first depths and counts, on both protocols
                assert r.watchFirstDepth(w) == depth and c[w][depth] == count, watch_cases.MP_NAMED[w]
    bare, _ = _bfs(proto, s.clone().clearWatches())
    assert _same_search(r, bare)


# ---- 3. table growth and the key-width restart: the census starts again from zero -----------------------------
@pytest.mark.parametrize("name", ["mp_c5_d8_named", "mpir_c5_d8_generic"])
def test_census_survives_table_growth(name):
    proto, s, _ = watch_cases.case(name)
    s.table_log2_slots = 10  # 1,024 slots for 17,320 states: rehashed at level boundaries
    r, st = _bfs(proto, s)
    assert st["table_rehashes"] >= 1
    assert r.per_depth == watch_cases.gold(name)["per_depth"] and r.watchCounts() == watch_cases.gold(name)["census"]


def test_census_survives_the_key_width_restart(monkeypatch, capfd):
    """As tests/test_gpu_table.py::test_key_width_restart: from 2^10 slots (b0 = 7) and DSL_KEY_RISK 15
    the growth to 2^12 buckets (2 * 12 - 7 > 15) restarts the search, after levels were counted."""
    monkeypatch.setenv("DSL_KEY_RISK", "15")
    monkeypatch.setenv("DSL_LEVEL_TRACE", "1")
    proto, s, _ = watch_cases.case("mp_c5_d8_named")
    s.table_log2_slots = 10
    r, st = _bfs(proto, s)
    assert "restart" in capfd.readouterr().err
    assert st["table_slots"] >= 2 * r.states
    assert r.per_depth == watch_cases.gold("mp_c5_d8_named")["per_depth"]
    assert r.watchCounts() == watch_cases.gold("mp_c5_d8_named")["census"]


# ---- 4. find mode: the level's re-run counts nothing ---------------------------------------------------------
@pytest.mark.parametrize("cap", [None, "0", "1"])
def test_find_mode_counts_nothing_twice(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("DSL_TERM_CAP", raising=False)
    else:
        monkeypatch.setenv("DSL_TERM_CAP", cap)  # 0: the terminal list keeps nothing, the find pass must run
    proto, s, _ = watch_cases.case("pp_1c10p_goal")
    fix = watch_cases.fixture("lab0", "lab0_1c10p_goal")
    r, st = _bfs(proto, s.maxTerminals(16))
    if cap == "0":
        assert st["terminal_finds"] >= 1
    assert r.endCondition() == EndCondition.GOAL_FOUND and r.per_depth == fix["per_depth"] and r.states == fix["states"]
    c = r.watchCounts()
    assert c == watch_cases.gold("pp_1c10p_goal")["census"]
    assert c[0][20] == 1 == r.numTerminals() and r.watchFirstDepth(0) == 20 and r.watchTotal(0) == 1


# ---- 5. a staged start over a dropped network ------------------------------------------------------------------
def test_dropped_network_and_depth_offset():
    mp = MultiPaxosIR(3, 2, "append-xy")
    dec = mp.message("Decision")
    leaf = dec.where(dec.field("slot") == 1)
    s = SearchSettings().addGoal(leaf)
    s.table_log2_slots = 20
    e = Engine(mp)
    try:
        s1 = e.bfs(mp.initial_state(), s).goalMatchingState()
        assert s1.depth() > 0 and S.message_matches(s1, leaf)
        s1.dropPendingMessages()  # every record, the Decision among them, is now only in the dropped set
        assert not [r for r in s1.records() if r not in s1.droppedMessages()]
        free = SearchSettings().maxDepth(s1.depth() + 2).addWatch(leaf).addWatch(leaf.negate())
        free.addWatch(mp.message("P2a").where().or_(leaf))
        free.table_log2_slots = 20
        r = e.bfs(s1, free)
        assert r.initial_depth == s1.depth() and len(r.per_depth) == 3 and r.per_depth[1] >= 1
        c = r.watchCounts()
        assert c[0] == r.per_depth and c[2] == r.per_depth  # by the dropped copy, on the host and in the kernels
        assert c[1] == [0] * 3
        assert r.watchFirstDepth(0) == s1.depth() and r.watchFirstDepth(1) is None
        assert r.watchTotal(0) == r.states
    finally:
        e.close()


# ---- 6. PB: the named network predicate (kNetPreds) and its raw-message restatement ----------------------------
def test_pb_named_network_predicate():
    proto, s, _ = watch_cases.case("pb_2s1c_d6")
    r, _ = _bfs(proto, s)
    c = r.watchCounts()
    assert r.per_depth == watch_cases.gold("pb_2s1c_d6")["per_depth"] and c == watch_cases.gold("pb_2s1c_d6")["census"]
    assert c[0] == c[1] and r.watchFirstDepth(0) == 1 and c[0][1] == 2  # the oracle's anchor


# ---- 7. refusals through the C ABI -------------------------------------------------------------------------------
def test_c_abi_refuses_a_bad_watch_and_keeps_the_old_ones():
    proto, s, _ = watch_cases.case("pp_1c10p_8w")
    gold = watch_cases.gold("pp_1c10p_8w")
    e = Engine(proto)
    try:
        assert e.bfs(proto.initial_state(), s).watchCounts() == gold["census"]
        bad = (_lib.dsl_predicate * 1)(_lib.dsl_predicate(S.PRED_FIELD, 0, S.field_arg0(S.field_desc(1, 30, 4), S.CMP_EQ, False), 1))
        assert e.lib.dsl_set_watches(e.handle, bad, 1, None, 0) == DSL_ERR_ARG
        assert b"straddles a 32-bit word" in e.lib.dsl_last_error()
        nine = (_lib.dsl_predicate * 9)(*[_lib.dsl_predicate(S.PRED_CLIENTS_DONE, 0, 0, 0)] * 9)
        assert e.lib.dsl_set_watches(e.handle, nine, 9, None, 0) == DSL_ERR_ARG
        cond = (_lib.dsl_predicate * 1)(_lib.dsl_predicate(S.PRED_REC_COND, 0, S.rec_arg0(0, 4, S.CMP_EQ), 1))
        assert e.lib.dsl_set_watches(e.handle, cond, 1, None, 0) == DSL_ERR_ARG
        assert b"DSL_PRED_REC_COND" in e.lib.dsl_last_error()
        # the engine kept its eight watches and still searches
        assert e.bfs(proto.initial_state(), s).watchCounts() == gold["census"]
        with pytest.raises(_lib.EngineError) as err:  # the same through the Python API
            e.bfs(proto.initial_state(), s.clone().clearWatches().addWatch(StatePredicate("bad", S.PRED_FIELD, bad[0].arg0, 1)))
        assert err.value.code == DSL_ERR_ARG and "dsl_set_watches" in str(err.value)
        # after a DFS and a replay there is no census
        goal = SearchSettings().addGoal(CLIENTS_DONE).addWatch(CLIENTS_DONE)
        g = e.bfs(proto.initial_state(), goal)
        assert g.endCondition() == EndCondition.GOAL_FOUND and g.watchCounts()[0][20] == 1
        n, total = ctypes.c_int32(0), ctypes.c_uint64(0)
        assert e.lib.dsl_watch_counts(e.handle, 0, None, 0, ctypes.byref(n), ctypes.byref(total)) == 0
        assert (n.value, total.value) == (21, 1)
        d = e.dfs(proto.initial_state(), goal.clone().maxDepth(30), probes=256, max_probes=256, seed=1)  # one launch
        assert d.watchCounts() == []
        assert e.lib.dsl_watch_counts(e.handle, 0, None, 0, ctypes.byref(n), ctypes.byref(total)) == 0
        assert (n.value, total.value) == (0, 0)
        assert e.bfs(proto.initial_state(), goal).watchCounts() == g.watchCounts()
        rp = e.replay(proto.initial_state(), goal, g.goalMatchingState().events())
        assert rp.endCondition() == EndCondition.GOAL_FOUND and rp.watchCounts() == []
        assert e.lib.dsl_watch_counts(e.handle, 0, None, 0, ctypes.byref(n), None) == 0 and n.value == 0
        assert e.bfs(proto.initial_state(), s).watchCounts() == gold["census"]
    finally:
        e.close()


def test_watches_are_refused_on_several_shards():
    proto, s, _ = watch_cases.case("mp_c5_d8_named")
    e = Engine(proto, virtual_shards=3, replicate_below=0)
    try:
        with pytest.raises(_lib.EngineError) as err:
            e.bfs(proto.initial_state(), s)
        assert err.value.code == DSL_ERR_ARG and "dsl_run" in str(err.value)
        assert "watches are not supported in a search over more than one shard" in str(err.value)
        r = e.bfs(proto.initial_state(), s.clone().clearWatches())  # the same engine, once the watches are cleared
        assert r.per_depth == watch_cases.gold("mp_c5_d8_named")["per_depth"] and r.watchCounts() == []
    finally:
        e.close()


# ---- 8. no watches --------------------------------------------------------------------------------------------
def test_no_watches_no_census():
    proto = PingPongIR(1, 10)
    s = SearchSettings().addInvariant(RESULTS_OK).addPrune(CLIENTS_DONE)
    s.table_log2_slots = 20
    e = Engine(proto)
    try:
        r = e.bfs(proto.initial_state(), s)
        fix = watch_cases.fixture("lab0", "lab0_1c10p_exhaustive")
        assert r.watchCounts() == [] and r.per_depth == fix["per_depth"] and r.states == fix["states"]
        assert getattr(e, "_set_watch_key", b"") == b""  # dsl_set_watches was never called
        n = ctypes.c_int32(5)
        assert e.lib.dsl_watch_counts(e.handle, 0, None, 0, ctypes.byref(n), None) == 0 and n.value == 0
    finally:
        e.close()
