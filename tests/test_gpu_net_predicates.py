"""User-written message predicates (MessagePattern.where -> DSL_PRED_NET) judged by the MI355X
kernels: pb.json restated on the engine (unsharded and over 3 virtual shards), searches over a
dropped network against the oracle run live with the NAMED predicate, a protocol whose kernels
stage no new records (Multi-Paxos: 64-bit records, 12 sends per step) against the oracle and the
host check, the smallest case (PingPongIR) through BFS, random DFS and replay, the equivalence of
the raw-message leaf with PB's named predicate and with a field leaf, and the C ABI's refusal of a
bad leaf."""
import ctypes

import pytest

import argmap
import net_cases
import oracle_util
from dslabs_amd import EndCondition, Engine, Search, SearchSettings, NONE_DECIDED, StatePredicate, _lib, message_matches
from dslabs_amd import search as S
from dslabs_amd.protocols import PB, MultiPaxosIR, PingPongIR
from test_gpu_dropped import _check
from test_net_predicates import REFUSALS, netcheck_build, netcheck_rows

pytestmark = pytest.mark.gpu
DSL_ERR_ARG = -1  # include/dslabs_hip.h dsl_status


def _bfs(proto, settings, start=None, **eng):
    e = Engine(proto, **eng)
    try:
        return e.bfs(start or proto.initial_state(), settings)
    finally:
        e.close()


# ---- 1. pb.json restated, on the engine ----------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
@pytest.mark.parametrize("name", net_cases.CASES)
def test_engine_matches_pb_golden_with_message_predicates(name, shards):
    """Every pb.json case (all seven use hasViewReply; none is left out): prunes, a goal, and
    initView's and(..., !...) trees."""
    gold, proto, settings = net_cases.case(name)
    r = _bfs(proto, settings, virtual_shards=shards, replicate_below=0 if shards else -1)
    assert r.endCondition().name == gold["end"]
    assert r.per_depth == gold["per_depth"]
    assert r.states == gold["states"]
    st = r.invariantViolatingState() or r.goalMatchingState()
    if gold["terminal_depth"] >= 0:
        assert st.depth() == gold["terminal_depth"]
    else:
        assert st is None and r.max_depth == gold["max_depth"]


# ---- 2. the dropped network ------------------------------------------------------------------------------
PB1 = ["--proto", "pb", "--servers", "2", "--clients", "1", "--workload", "putget"]


def _view_reply_1_1_null(proto):
    """hasViewReply(1, server1, null) over the hand-written PB's record (pb.hpp: type = m >> 60,
    2 = ViewReply; the view = m & 0xff = num | p << 4 | b << 6)."""
    m = proto.raw_message("ViewReply")
    return m.where(m.raw_field(60, 4) == 2, m.raw_field(0, 8) == (1 | 1 << 4 | 0 << 6))


@pytest.mark.parametrize("form,extra,end", [
    ("inv", ["--inv", "!hasViewReply:1:1:-1"], "INVARIANT_VIOLATED"),
    ("or", ["--inv", "or(!hasViewReply:1:1:-1,NONE_DECIDED)"], "INVARIANT_VIOLATED"),
    ("prune", ["--prune", "hasViewReply:1:1:-1", "--network-off"], "SPACE_EXHAUSTED"),
])
def test_dropped_network_with_message_predicates(form, extra, end):
    """test_gpu_dropped's hasViewReply:1:1:-1 flows with the generic leaf: after the ViewReply of
    View(1, server1, null) is dropped the leaf still sees it -- on the host (the start state's own
    check) and in the kernels (with the network off only the dropped copy prunes the successors).
    The oracle starts from the same trace with the NAMED predicate."""
    proto = argmap.protocol(PB1)
    leaf = _view_reply_1_1_null(proto)
    r1 = Search.bfs(proto.initial_state(), SearchSettings().addInvariant(argmap.predicate(proto, "RESULTS_OK")).addGoal(leaf))
    assert r1.endCondition() == EndCondition.GOAL_FOUND
    s1 = r1.goalMatchingState()
    assert message_matches(s1, leaf)
    s1.dropPendingMessages()
    assert s1.droppedMessages() and message_matches(s1, leaf)  # network() keeps the dropped records
    a2 = PB1 + ["--inv", "RESULTS_OK"] + extra + ["--max-depth", str(s1.depth() + 12)]
    s2 = argmap.settings(PB1 + ["--inv", "RESULTS_OK", "--max-depth", str(s1.depth() + 12)], proto)
    if form == "inv":
        s2.addInvariant(leaf.negate())
    elif form == "or":
        s2.addInvariant(leaf.negate().or_(NONE_DECIDED))
    else:
        s2.addPrune(leaf).networkActive(False)
    r2 = Search.bfs(s1, s2)
    assert r2.endCondition().name == end
    if form == "inv":  # the start state itself violates it (its dropped ViewReply)
        assert r2.invariantViolatingState().depth() == s1.depth()
    if form == "prune":  # every successor is pruned by the dropped reply alone
        assert len(r2.per_depth) == 2
    _check(r2, a2, s1, s1.trace() + ["#DROP"])


MP = MultiPaxosIR(3, 2, "append-xy")


def _decision_slot1():
    dec = MP.message("Decision")
    return dec.where(dec.field("slot") == 1)


def test_dropped_records_reach_kernels_that_stage_no_sends():
    """Multi-Paxos has no named network predicate (no kNetPreds): its dropped records are uploaded
    for the generic leaf all the same. After the goal's Decision is dropped, the leaf as a prune
    cuts every successor of the start state, by the dropped copy alone."""
    leaf = _decision_slot1()
    s = SearchSettings().addGoal(leaf)
    s.table_log2_slots = 20
    e = Engine(MP)
    try:
        s1 = e.bfs(MP.initial_state(), s).goalMatchingState()
        n = len(message_matches(s1, leaf))
        assert n >= 1
        s1.dropPendingMessages()
        assert len(message_matches(s1, leaf)) == n and len(s1.droppedMessages()) == len(s1.records())
        free = SearchSettings().maxDepth(s1.depth() + 1)
        free.table_log2_slots = 20
        want = e.bfs(s1, free).per_depth  # timers only: the network is empty
        assert len(want) == 2 and want[1] >= 1
        cut = SearchSettings().addPrune(leaf).maxDepth(s1.depth() + 3)
        cut.table_log2_slots = 20
        r = e.bfs(s1, cut)
        assert r.endCondition() == EndCondition.SPACE_EXHAUSTED and r.per_depth == want
    finally:
        e.close()


# ---- 3. a protocol without kNetPreds: 64-bit records, 12 sends per step ----------------------------------------
def _p2a_from_server2():
    return MP.message("P2a", frm="server2").where()


MP_CASES = {
    # name: (settings, netcheck scenario, is a goal)
    "goal_decision": (lambda: SearchSettings().addGoal(_decision_slot1()), "mp_goal_decision", True),
    "inv_no_p2a": (lambda: SearchSettings().addInvariant(_p2a_from_server2().negate()), "mp_inv_p2a", False),
}


@pytest.fixture(scope="module")
def netcheck():
    return {r["scenario"]: r for r in netcheck_rows(netcheck_build("plain"))[:-1]}


@pytest.fixture(scope="module")
def mp_unconstrained():
    """The oracle's unconstrained per-depth counts, run live, as deep as the two cases end."""
    return oracle_util.run("bfs", MP.oracle_args() + ["--max-depth", "5"], timeout=120)["per_depth"]


@pytest.mark.parametrize("name", sorted(MP_CASES))
def test_multipaxos_message_predicates(name, netcheck, mp_unconstrained):
    build, scenario, goal = MP_CASES[name]
    settings = build().maxTerminals(64)
    settings.table_log2_slots = 20
    r = _bfs(MP, settings)
    host = netcheck[scenario]
    assert r.endCondition() == (EndCondition.GOAL_FOUND if goal else EndCondition.INVARIANT_VIOLATED)
    st = r.goalMatchingState() if goal else r.invariantViolatingState()
    depth = st.depth()
    assert 1 <= depth <= 5
    assert r.per_depth[:depth] == mp_unconstrained[:depth]      # the completed levels
    assert depth == host["terminal_depth"] and r.numTerminals() == host["terminal"] == len(r.terminals())
    leaf = settings.goals()[0] if goal else settings.invariants()[0]
    fired = (r.goalMatched() if goal else r.invariantViolated()).predicate
    assert fired is leaf
    for end, pred, t in r.terminals():
        assert end == r.endCondition() and pred.predicate is leaf and t.depth() == depth
        assert message_matches(t, leaf)  # a matching message, decoded from the state's bytes
    # no state before the terminal level held one: the search would have ended there
    rep = oracle_util.replay(MP.oracle_args(), st.trace())
    assert rep["ok"], rep["error"]
    assert rep["depth"] == depth


# ---- 4. the smallest case ------------------------------------------------------------------------------------
def test_pingpong_goal_bfs_dfs_and_replay():
    """PingPongIR, one client, 32-bit records. lab0_1c10p_goal finds all ten results at depth 20:
    two steps a ping (the request's delivery sends the reply, the reply's delivery the next
    request). `_results` reaches length 2 at depth 4, the delivery that sends PingRequest(3); the
    next step delivers it and sends PongReply(3): depth 2 * 2 + 1 = 5."""
    import field_cases
    gold = field_cases.gold("lab0", "lab0_1c10p_goal")
    per_ping = gold["terminal_depth"] // 10
    assert per_ping == 2
    depth = per_ping * (3 - 1) + 1
    proto = PingPongIR(1, 10)
    pong = proto.message("PongReply")
    leaf = pong.where(pong.field("value") == 3)
    s = SearchSettings().addGoal(leaf).maxTimeSecs(60)
    s.table_log2_slots = 20
    r = Search.bfs(proto.initial_state(), s)
    assert r.endCondition() == EndCondition.GOAL_FOUND and r.goalMatched().predicate is leaf
    st = r.goalMatchingState()
    assert st.depth() == depth and r.per_depth == gold["per_depth"][:depth + 1]
    assert len(message_matches(st, leaf)) == 1
    rep = Search.replay(proto.initial_state(), s, st.events())
    assert rep.endCondition() == EndCondition.GOAL_FOUND and rep.goalMatchingState().depth() == depth
    d = Search.dfs(proto.initial_state(), s.maxDepth(12), probes=4096, seed=5)
    assert d.endCondition() == EndCondition.GOAL_FOUND and d.goalMatched().predicate is leaf
    dst = d.goalMatchingState()
    assert dst.depth() >= depth and message_matches(dst, leaf)
    rep = Search.replay(proto.initial_state(), s, dst.events())
    assert rep.endCondition() == EndCondition.GOAL_FOUND


# ---- 5. raw-message leaf == named predicate == field leaf ------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_raw_message_leaf_equals_named_predicate_and_field_leaf(n):
    """On the hand-written PB, hasViewReply(n) is the viewserver's maxSent >= n (pb.hpp: 4 bits at
    bit 15 of word 0): the named predicate, the raw-message leaf and the field leaf give the same
    search, down to the listed terminals' bytes."""
    proto = PB(2, 1, "putget")
    m = proto.raw_message("ViewReply")
    forms = {
        "named": proto.predicate(f"hasViewReply:{n}"),
        "message": m.where(m.raw_field(60, 4) == 2, m.raw_field(0, 4) >= n),
        "field": proto.raw_field("viewserver", 15, 4) >= n,
    }
    got = {}
    for form, pred in forms.items():
        s = SearchSettings().addGoal(pred).maxTerminals(64)
        s.table_log2_slots = 20
        r = _bfs(proto, s)
        assert r.endCondition() == EndCondition.GOAL_FOUND and r.numTerminals() >= 1
        got[form] = (r.per_depth, r.states, r.numTerminals(), [(t.depth(), t.packed) for _, _, t in r.terminals()])
        for _, _, t in r.terminals():
            assert message_matches(t, forms["message"])
    assert got["message"] == got["named"] == got["field"]


# ---- 6. the C ABI refuses a bad leaf and the engine goes on -----------------------------------------------------
def test_c_abi_refuses_bad_network_leaves_and_still_searches():
    proto = PingPongIR(1, 10)  # 32-bit records
    pong = proto.message("PongReply")
    good = SearchSettings().addGoal(pong.where(pong.field("value") == 3))
    good.table_log2_slots = 20
    e = Engine(proto)
    try:
        first = e.bfs(proto.initial_state(), good)
        assert first.endCondition() == EndCondition.GOAL_FOUND
        for pred, why in REFUSALS:
            # alone, and as a combinator's operand (other pool entries then follow the leaf's own, so
            # a range past them may be named as an entry that is no condition instead)
            for s, exact in ((SearchSettings().addGoal(pred), True),
                             (SearchSettings().addInvariant(good.goals()[0].or_(pred)), False)):
                with pytest.raises(_lib.EngineError) as err:
                    e.bfs(proto.initial_state(), s)
                assert err.value.code == DSL_ERR_ARG
                msg = str(err.value)
                assert "dsl_set_settings" in msg and ("network predicate" in msg or "record condition" in msg)
                assert why in msg or not exact
        # dsl_set_settings straight through ctypes: DSL_ERR_ARG and a dsl_last_error text
        enc = SearchSettings().addPrune(REFUSALS[4][0])._encode(proto.initial_state())
        assert e.lib.dsl_set_settings(e.handle, ctypes.byref(enc)) == DSL_ERR_ARG
        assert b"width outside 1..32" in e.lib.dsl_last_error()
        # the engine kept the settings it had (a run without new settings), and takes new ones
        res = ctypes.POINTER(_lib.dsl_result)()
        assert e.lib.dsl_run(e.handle, ctypes.byref(res)) == 0
        assert res.contents.end_condition == 2 and res.contents.terminal_depth == first.goalMatchingState().depth()
        assert [res.contents.per_depth[i] for i in range(res.contents.n_levels)] == first.per_depth
        e.lib.dsl_result_free(res)
        again = e.bfs(proto.initial_state(), good)
        assert again.endCondition() == EndCondition.GOAL_FOUND and again.per_depth == first.per_depth
        assert isinstance(REFUSALS[0][0], StatePredicate) and S.PRED_NET == 951
    finally:
        e.close()
