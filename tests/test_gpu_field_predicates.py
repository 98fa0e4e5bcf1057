"""User-written field predicates (FieldRef comparisons -> DSL_PRED_FIELD) judged by the MI355X
kernels: the golden fixtures restated, PaxosTest's lab3 predicates restated on the IR-generated
Multi-Paxos against the oracle run live with the NAMED predicates, field-field compares, random
DFS, and the C ABI's refusal of bad descriptors."""
import ctypes

import pytest

import field_cases
import oracle_util
from dslabs_amd import (EndCondition, Engine, Search, SearchSettings, StatePredicate, _lib, allOf, anyOf,
                        field_value)
from dslabs_amd import search as S
from dslabs_amd.protocols import MultiPaxosIR, PingPongIR

pytestmark = pytest.mark.gpu
DSL_ERR_ARG = -1  # include/dslabs_hip.h dsl_status


def _bfs(proto, settings, **eng):
    e = Engine(proto, **eng)
    try:
        return e.bfs(proto.initial_state(), settings)
    finally:
        e.close()


# ---- 4. the golden fixtures, restated, on the engine ---------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
@pytest.mark.parametrize("name", sorted(field_cases.CASES))
def test_engine_matches_golden_with_field_predicates(name, shards):
    gold, proto, settings = field_cases.case(name)
    r = _bfs(proto, settings, virtual_shards=shards, replicate_below=0 if shards else -1)
    assert r.endCondition().name == gold["end"]
    assert r.per_depth == gold["per_depth"]
    assert r.states == gold["states"]
    st = r.invariantViolatingState() or r.goalMatchingState()
    if gold["terminal_depth"] >= 0:
        assert st.depth() == gold["terminal_depth"]
    else:
        assert st is None and r.max_depth == gold["max_depth"]


# ---- 5. PaxosTest's lab3 predicates restated over the log's sub-fields -------------------------------
MP = MultiPaxosIR(3, 2, "append-xy")
STATUS = {"EMPTY": 0, "ACCEPTED": 1, "CHOSEN": 2}


def has_status(server, slot, status):
    """hasStatus(a, i, s) (ir/specs/multipaxos.py _has_status): log[i - 1]'s status bits."""
    return MP.field(server, "log", slot - 1).bits(0, 2) == STATUS[status]


def has_command_x(server, slot):
    """hasCommand(a, i, X) (_has_command): the slot is not EMPTY and holds Paxos command 1 --
    client1's first command, append-xy's APPEND X (command 0 is the no-op, 4 client2's APPEND Y)."""
    e = MP.field(server, "log", slot - 1)
    return (e.bits(0, 2) != 0).and_(e.bits(8, 3) == 1)


def _lab3():
    chosen1 = has_status("server1", 1, "CHOSEN")
    return {
        # name: (oracle arguments, settings, holds(state) of the fired predicate, its index, the oracle's name of it)
        "goal_has_status": (["--goal", "hasStatus:server2:1:CHOSEN"],
                            SearchSettings().addGoal(has_status("server2", 1, "CHOSEN")),
                            lambda st: field_value(st, MP.field("server2", "log", 0).bits(0, 2)) == 2, 0, "has status"),
        "inv_implies": (["--inv", "implies(hasStatus:server1:1:CHOSEN,hasCommand:server1:1:X)", "--inv", "slotValid:1"],
                        SearchSettings().addInvariant(chosen1.implies(has_command_x("server1", 1)))
                        .addInvariant(MP.predicate("slotValid:1")),
                        lambda st: (field_value(st, MP.field("server1", "log", 0).bits(0, 2)) != 2 or
                                    field_value(st, MP.field("server1", "log", 0).bits(8, 3)) == 1), 0,
                        "(has status) → (has command)"),
        "inv_not_accepted": (["--inv", "!hasStatus:server2:1:ACCEPTED"],
                             SearchSettings().addInvariant(has_status("server2", 1, "ACCEPTED").negate()),
                             lambda st: field_value(st, MP.field("server2", "log", 0).bits(0, 2)) != 1, 0,
                             "¬(has status)"),
    }


# what the issue pins of the oracle's answers: (terminal depth, states, terminals on the level)
PINNED = {"goal_has_status": (4, 298, 4), "inv_implies": (3, 91, None), "inv_not_accepted": (2, 25, 2)}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_lab3_predicates_restated_match_the_oracle(name):
    from test_ir import _mp_oracle_args
    oargs, settings, holds, index, oracle_name = _lab3()[name]
    base = ["--proto", "multipaxos", "--workload", "append-xy"]
    want = oracle_util.run("bfs", base + oargs + ["--finish-level"], timeout=120)
    depth, states, nterm = PINNED[name]
    assert (want["terminals"][0]["depth"], want["states"]) == (depth, states)
    assert nterm is None or want["num_terminals"] == nterm
    assert all(t["predicate"] == oracle_name for t in want["terminals"])  # the predicate at `index`
    settings.table_log2_slots = 20
    r = _bfs(MP, settings.maxTerminals(64))
    goal = want["end"] == "GOAL_FOUND"
    assert r.endCondition().name == want["end"]
    assert r.per_depth == want["per_depth"] and r.states == want["states"]
    st = r.goalMatchingState() if goal else r.invariantViolatingState()
    assert st.depth() == depth
    fired = (r.goalMatched() if goal else r.invariantViolated()).predicate
    assert fired is (settings.goals() if goal else settings.invariants())[index]
    assert r.numTerminals() == want["num_terminals"] and len(r.terminals()) == want["num_terminals"]
    for end, pred, t in r.terminals():
        assert end == r.endCondition() and pred.predicate is fired and t.depth() == depth
        assert holds(t) == goal  # the goal holds / the invariant is false, decoded from the state's bytes
    # the reported terminal's trace replays on the oracle, where the NAMED predicate says the same
    rep = oracle_util.replay(_mp_oracle_args(MP, oargs), st.trace())
    assert rep["ok"], rep["error"]
    assert rep["depth"] == depth
    if goal:
        assert rep["goals"][index]["value"]
    else:
        assert not rep["invariants"][index]["value"]


# ---- 6. field-field compare == its expansion over the constants ----------------------------------------
def _leaders(form):
    a, b = MP.field("server1", "leader"), MP.field("server2", "leader")
    if form == "field":
        return a == b
    return anyOf([(a == v).and_(b == v) for v in range(4)])  # leader: 2 bits


@pytest.mark.parametrize("kind", ["invariant", "goal"])
def test_field_field_compare_equals_its_expansion(kind):
    """server1.leader == server2.leader as one field-field leaf and as anyOf(v: both == v): the same
    search, down to the listed terminal states' bytes. The goal form adds "server1 and server2 have
    left round 0" (the initial state has equal leaders)."""
    got = []
    for form in ("field", "expanded"):
        s = SearchSettings().maxTerminals(64)
        s.table_log2_slots = 20
        if kind == "invariant":
            s.addInvariant(_leaders(form))
        else:
            moved = [MP.field("server1", "round") >= 1, MP.field("server2", "round") > 0]
            s.addGoal(allOf([_leaders(form)] + moved)).maxDepth(8)
        r = _bfs(MP, s)
        got.append((r.endCondition(), r.per_depth, r.states, r.numTerminals(),
                    [(e, t.depth(), t.packed) for e, _, t in r.terminals()]))
        want_end = EndCondition.INVARIANT_VIOLATED if kind == "invariant" else EndCondition.GOAL_FOUND
        assert r.endCondition() == want_end and r.numTerminals() >= 1 and len(r.terminals()) == min(64, r.numTerminals())
        for _, _, t in r.terminals():
            l1, l2 = (field_value(t, MP.field(a, "leader")) for a in ("server1", "server2"))
            if kind == "invariant":
                assert l1 != l2
            else:
                assert l1 == l2 and field_value(t, MP.field("server1", "round")) >= 1 and \
                    field_value(t, MP.field("server2", "round")) >= 1
    assert got[0] == got[1]
    assert got[0][4][0][1] >= 1  # not the initial state


# ---- 7. random DFS ---------------------------------------------------------------------------------------
def test_dfs_with_a_field_goal():
    proto = PingPongIR(1, 2)
    done = proto.length("client1", "_results") == 2
    s = SearchSettings().addGoal(done).maxDepth(12).maxTimeSecs(60)
    r = Search.dfs(proto.initial_state(), s, probes=4096, seed=3)
    assert r.endCondition() == EndCondition.GOAL_FOUND
    st = r.goalMatchingState()
    assert r.goalMatched().predicate is done and st.depth() >= 4  # lab0_1c2p_goal: BFS finds it at depth 4
    assert field_value(st, proto.length("client1", "_results")) == 2
    assert [field_value(st, proto.field("client1", "_results", j)) for j in range(2)] == [1, 2]


# ---- 8. the C ABI refuses a bad descriptor and the engine goes on -----------------------------------------
def _leaf(arg0, arg1=0):
    return StatePredicate("bad", S.PRED_FIELD, arg0, arg1)


def test_c_abi_refuses_bad_descriptors_and_still_searches():
    proto = PingPongIR(1, 10)  # 2 nodes of 6 words
    d = S.field_desc
    bad = [(_leaf(S.field_arg0(d(2, 0, 4), S.CMP_EQ, False)), "node index"),
           (_leaf(S.field_arg0(d(1, 0, 33), S.CMP_EQ, False)), "width outside 1..32"),
           (_leaf(S.field_arg0(d(1, 0, 0), S.CMP_EQ, False)), "width outside 1..32"),
           (_leaf(S.field_arg0(d(1, 30, 4), S.CMP_EQ, False)), "straddles"),
           (_leaf(S.field_arg0(d(1, 192, 1), S.CMP_EQ, False)), "beyond the node"),
           (_leaf(S.field_arg0(d(1, 0, 4), 7, False)), "unknown comparison"),
           (_leaf(S.field_arg0(d(1, 0, 4), S.CMP_LT, True), d(1, 160, 32) + 32), "right operand")]
    gold, _, good = field_cases.case("lab0_1c10p_goal")
    e = Engine(proto)
    try:
        first = e.bfs(proto.initial_state(), good)
        assert first.per_depth == gold["per_depth"]
        for pred, why in bad:
            for s in (SearchSettings().addGoal(pred), SearchSettings().addInvariant(good.goals()[0].or_(pred))):
                with pytest.raises(_lib.EngineError) as err:
                    e.bfs(proto.initial_state(), s)
                assert err.value.code == DSL_ERR_ARG
                assert "dsl_set_settings" in str(err.value) and "field predicate" in str(err.value) and why in str(err.value)
        # dsl_set_settings straight through ctypes: DSL_ERR_ARG and a dsl_last_error text
        enc = SearchSettings().addPrune(bad[3][0])._encode(proto.initial_state())
        assert e.lib.dsl_set_settings(e.handle, ctypes.byref(enc)) == DSL_ERR_ARG
        assert b"straddles a 32-bit word" in e.lib.dsl_last_error()
        # the engine kept the settings it had, and takes new ones
        again = e.bfs(proto.initial_state(), good)
        assert again.endCondition() == EndCondition.GOAL_FOUND and again.per_depth == gold["per_depth"]
        gold2, _, prune = field_cases.case("lab0_1c10p_exhaustive")
        assert e.bfs(proto.initial_state(), prune).per_depth == gold2["per_depth"]
    finally:
        e.close()
