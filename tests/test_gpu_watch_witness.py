"""Witnesses of the watches (SearchSettings.addWatch(p, witness=True)) selected by the MI355X
kernels: every witness against tests/golden/witness.json (the host truth of
tests/hostcheck/witnesscheck.cpp), against the engine's own goal search with maxTerminals and against
the oracle's replay and finished level, with the search and the census unchanged; table growth and
the key-width restart, the level that ends a search, determinism, a staged start over a dropped
network that feeds the next stage, the named network predicates, refusals and lifetimes."""
import ctypes

import pytest

import oracle_util
import watch_cases
import witness_cases
from dslabs_amd import CLIENTS_DONE, EndCondition, Engine, SearchSettings, _lib
from dslabs_amd import search as S
from dslabs_amd.protocols import MultiPaxosIR
from test_ir import _mp_oracle_args

pytestmark = pytest.mark.gpu
DSL_ERR_ARG = -1  # include/dslabs_hip.h dsl_status
INVS = ["--inv", "RESULTS_OK", "--inv", "LOGS_CONSISTENT_ALL_SLOTS", "--inv", "APPENDS_LINEARIZABLE"]
LIST = ["--finish-level", "--print-states", "--max-terminals", "100000"]


def _bfs(proto, settings, state=None, **eng):
    e = Engine(proto, **eng)
    try:
        return e.bfs(state if state is not None else proto.initial_state(), settings), e.kernel_stats()
    finally:
        e.close()


def _same_search(a, b):
    return (a.endCondition(), a.states, a.per_depth, a.max_depth, a.successors) == \
        (b.endCondition(), b.states, b.per_depth, b.max_depth, b.successors)


def _packed(r, n):
    return [None if r.watchWitness(i) is None else r.watchWitness(i).packed for i in range(n)]


def _gold_packed(name):
    return [witness_cases.gold_state(name, w) for w in range(len(witness_cases.gold(name)["witnesses"]))]


def _check_against_fixture(name, r):
    """Every witness is the fixture's state, at watchFirstDepth, with a trace of that many events."""
    gold = witness_cases.gold(name)["witnesses"]
    for w, g in enumerate(gold):
        wit = r.watchWitness(w)
        if g["first_depth"] < 0:
            assert wit is None and r.watchFirstDepth(w) is None
            continue
        assert wit is not None, (name, w)
        print(name, w, "depth", wit.depth(), "fixture", g["first_depth"], "holders", g["holders"])
        assert wit.depth() == r.watchFirstDepth(w) == g["first_depth"]
        assert len(wit.trace()) == len(wit.events()) == wit.depth() - r.initial_depth == g["trace_len"]
        assert wit.packed == bytes.fromhex(g["state"]), (name, w)


# ---- 1. lab0: eight witnesses in one search; a watch nothing holds, a watch the start state holds ------------
def test_pingpong_witnesses():
    proto, s, _ = witness_cases.case("pp_1c10p_8w")
    r, _ = _bfs(proto, s)
    plain, _ = _bfs(proto, watch_cases.case("pp_1c10p_8w")[1])
    assert _same_search(r, plain) and r.watchCounts() == plain.watchCounts() == watch_cases.gold("pp_1c10p_8w")["census"]
    assert [plain.watchWitness(i) for i in range(8)] == [None] * 8
    _check_against_fixture("pp_1c10p_8w", r)
    start = proto.initial_state()._packed_now()
    for w in (2, 3, 6):  # true on the start state: the start state itself, no event
        assert r.watchWitness(w).packed == start and r.watchWitness(w).trace() == [] and r.watchWitness(w).depth() == 0
    with pytest.raises(ValueError):
        r.watchWitness(8)
    proto, s, _ = witness_cases.case("pp_1c10p_extra")
    x, _ = _bfs(proto, s)
    bare, _ = _bfs(proto, s.clone().clearWatches())
    assert _same_search(x, bare)
    _check_against_fixture("pp_1c10p_extra", x)
    assert x.watchWitness(0) is None and x.watchTotal(0) == 0               # no reachable state holds it
    assert x.watchWitness(1).packed == start and x.watchWitness(1).trace() == []
    assert x.watchWitness(2).packed == r.watchWitness(0).packed and x.watchWitness(2).depth() == 20


# ---- 2. mp_c5_d8: selection across waves and workgroups, the maxDepth level, inside the level queue ---------
def _oracle_args(name, proto, watch):
    rest = ["--goal", watch, "--max-depth", "9"]
    if name == "mp_c5_d8_named":
        return ["--proto", "multipaxos", "--workload", "append-xy"] + INVS + rest
    return _mp_oracle_args(proto, INVS + rest)


_mp_results = {}


def _mp_witnessed(name):
    """The witnessed search of a Multi-Paxos case, run once for the tests of its seven watches."""
    if name not in _mp_results:
        proto, s, _ = witness_cases.case(name)
        _mp_results[name] = (proto, s, _bfs(proto, s)[0])
    return _mp_results[name]


@pytest.mark.parametrize("name", ["mp_c5_d8_named", "mpir_c5_d8_named"])
def test_multipaxos_witnesses(name):
    proto, s, r = _mp_witnessed(name)
    plain, _ = _bfs(proto, watch_cases.case(name)[1])
    assert _same_search(r, plain) and r.watchCounts() == plain.watchCounts() == watch_cases.gold(name)["census"]
    assert r.per_depth == watch_cases.fixture("multipaxos", "mp_c5_d8")["per_depth"]
    _check_against_fixture(name, r)


@pytest.mark.parametrize("w", range(len(watch_cases.MP_NAMED)))
@pytest.mark.parametrize("name", ["mp_c5_d8_named", "mpir_c5_d8_named"])
def test_multipaxos_witness_is_the_goal_searches_first_state(name, w):
    proto, s, r = _mp_witnessed(name)
    wit, watch = r.watchWitness(w), s.watches()[w]
    # the engine's own goal search: same invariants, the watch as the goal, every terminal listed
    g, _ = _bfs(proto, watch_cases._mp_settings(proto).maxDepth(9).addGoal(watch).maxTerminals(64))
    assert g.endCondition() == EndCondition.GOAL_FOUND
    assert g.numTerminals() == witness_cases.gold(name)["witnesses"][w]["holders"]
    assert g.goalMatchingStates()[0].packed == wit.packed and g.goalMatchingStates()[0].depth() == wit.depth()
    # the oracle: the trace replays to a goal state of that depth with every invariant holding, one
    # of the states of the oracle's finished level
    oargs = _oracle_args(name, proto, watch_cases.MP_NAMED[w])
    rep = oracle_util.replay(oargs, wit.trace())
    assert rep["ok"] and not rep["exception"] and rep["depth"] == wit.depth()
    assert len(rep["invariants"]) == 3 and all(i["value"] and not i["threw"] for i in rep["invariants"])
    assert rep["goals"][0]["value"]
    want = oracle_util.run("bfs", oargs + LIST, timeout=300)
    assert want["end"] == "GOAL_FOUND" and want["num_terminals"] == g.numTerminals()
    assert rep["state"] in {t["state"] for t in want["terminals"]}


# ---- 3. generic leaves: the witnesses decode, and restatements pick the named watch's state -------------------
def test_generic_watches_decode_on_their_witnesses():
    name = "mpir_c5_d8_generic"
    proto, s, _ = witness_cases.case(name)
    e = Engine(proto)
    try:
        r = e.bfs(proto.initial_state(), s)
        _check_against_fixture(name, r)
        ws = s.watches()
        for w in (0, 1, 2):  # field leaves: hasStatus over the log's status bits
            server, slot, status = watch_cases.MP_GENERIC[w][1].split(":")[1:]
            assert S.field_value(r.watchWitness(w), proto.field(server, "log", int(slot) - 1).bits(0, 2)) == watch_cases.STATUS[status]
        for w in (3, 4):     # message leaves: a matching record is in the witness's network()
            assert S.message_matches(r.watchWitness(w), ws[w])
        for w, watch in enumerate(ws):  # each witness is the first terminal of the goal search
            g = e.bfs(proto.initial_state(), watch_cases._mp_settings(proto).maxDepth(9).addGoal(watch).maxTerminals(64))
            assert g.goalMatchingStates()[0].packed == r.watchWitness(w).packed, w
        assert r.watchWitness(1).packed == r.watchWitness(6).packed  # the field leaf and the named leaf, one search
        named = _gold_packed("mpir_c5_d8_named")
        for k, (_, restates) in enumerate(watch_cases.MP_GENERIC):
            if restates:
                assert r.watchWitness(k).packed == named[watch_cases.MP_NAMED.index(restates)], restates
    finally:
        e.close()


# ---- 4. table growth and the key-width restart: the witnesses are found again -----------------------------------
def test_witnesses_survive_table_growth():
    proto, s, _ = witness_cases.case("mp_c5_d8_named")
    s.table_log2_slots = 10  # 1,024 slots for 17,320 states: rehashed at level boundaries
    r, st = _bfs(proto, s)
    assert st["table_rehashes"] >= 1
    assert r.watchCounts() == watch_cases.gold("mp_c5_d8_named")["census"]
    assert _packed(r, 7) == _gold_packed("mp_c5_d8_named")


def test_witnesses_survive_the_key_width_restart(monkeypatch, capfd):
    monkeypatch.setenv("DSL_KEY_RISK", "15")
    monkeypatch.setenv("DSL_LEVEL_TRACE", "1")
    proto, s, _ = witness_cases.case("mp_c5_d8_named")
    s.table_log2_slots = 10
    r, _ = _bfs(proto, s)
    assert "restart" in capfd.readouterr().err
    assert r.watchCounts() == watch_cases.gold("mp_c5_d8_named")["census"]
    _check_against_fixture("mp_c5_d8_named", r)


# ---- 5. the level that ends the search produces the witness -------------------------------------------------------
@pytest.mark.parametrize("cap", [None, "0", "1"])
def test_terminal_level_gives_the_goal_state(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("DSL_TERM_CAP", raising=False)
    else:
        monkeypatch.setenv("DSL_TERM_CAP", cap)
    proto, s, _ = witness_cases.case("pp_1c10p_goal")
    r, _ = _bfs(proto, s)
    fix = watch_cases.fixture("lab0", "lab0_1c10p_goal")
    assert r.endCondition() == EndCondition.GOAL_FOUND and r.per_depth == fix["per_depth"] and r.states == fix["states"]
    assert r.watchCounts() == watch_cases.gold("pp_1c10p_goal")["census"]
    _check_against_fixture("pp_1c10p_goal", r)
    assert r.watchWitness(0).packed == r.goalMatchingState().packed and r.watchWitness(0).depth() == 20
    assert r.watchWitness(0).trace() == r.goalMatchingState().trace()  # one state, one parent chain


# ---- 6. determinism --------------------------------------------------------------------------------------------------
def test_witnesses_are_deterministic():
    proto, s, _ = witness_cases.case("mp_c5_d8_named")
    want = _gold_packed("mp_c5_d8_named")
    e = Engine(proto)
    try:
        for _ in range(3):
            assert _packed(e.bfs(proto.initial_state(), s), 7) == want
    finally:
        e.close()
    assert _packed(_bfs(proto, s)[0], 7) == want


# ---- 7. a staged start over a dropped network; the witness starts the next stage ---------------------------------------
def test_dropped_network_depth_offset_and_the_next_stage():
    mp = MultiPaxosIR(3, 2, "append-xy")
    dec = mp.message("Decision")
    leaf = dec.where(dec.field("slot") == 1)
    s = SearchSettings().addGoal(leaf)
    s.table_log2_slots = 20
    e = Engine(mp)
    try:
        s1 = e.bfs(mp.initial_state(), s).goalMatchingState()
        s1.dropPendingMessages()  # the Decision is now only in the dropped set
        # one watch per other message type: a type with a dropped copy holds on the start state, a
        # type first sent by a timer of the emptied network (only timers are left to fire) holds later
        kinds = [mp.message(k).where() for k in ("Heartbeat", "P1a", "P1b", "P2a", "Reply", "Request")]
        free = SearchSettings().maxDepth(s1.depth() + 2).addWatch(leaf, witness=True).addWatch(leaf.negate(), witness=True)
        for k in kinds:
            free.addWatch(k, witness=True)
        free.table_log2_slots = 20
        r = e.bfs(s1, free)
        assert r.initial_depth == s1.depth()
        held = r.watchWitness(0)  # held by the dropped copy: the start state, at initial_depth
        assert held.packed == s1.packed and held.depth() == s1.depth() and held.events() == []
        assert held.droppedMessages() == s1.droppedMessages() and S.message_matches(held, leaf)
        assert r.watchWitness(1) is None
        for w in range(2, 8):
            wit, first = r.watchWitness(w), r.watchFirstDepth(w)
            print("watch", w, "first depth", first)
            assert (wit is None) == (first is None) and (wit is None or wit.depth() == first)
            if first == r.initial_depth:
                assert wit.packed == s1.packed and wit.events() == []
        hit_later = [w for w in range(2, 8) if (r.watchFirstDepth(w) or 0) > r.initial_depth]
        assert hit_later  # some message type is first sent after the staged start
        later, p2a = r.watchWitness(hit_later[0]), kinds[hit_later[0] - 2]
        assert later.depth() > r.initial_depth
        assert len(later.events()) == later.depth() - r.initial_depth and S.message_matches(later, p2a)
        assert later.droppedMessages() == s1.droppedMessages() and later.trace()[:s1.depth()] == s1.trace()
        # the next stage starts at the witness
        nxt = SearchSettings().maxDepth(later.depth() + 1)
        nxt.table_log2_slots = 20
        r2 = e.bfs(later, nxt)
        assert r2.initial_depth == later.depth() and r2.per_depth[0] == 1 and len(r2.per_depth) == 2
        # ... and replaying the witness's events from the stage's start state reaches it
        rp = e.replay(s1, SearchSettings(), later.events())
        assert rp.lastState().packed == later.packed
    finally:
        e.close()


# ---- 8. PB: the named network predicate (kNetPreds) ---------------------------------------------------------------------
def test_pb_named_network_predicate_witness():
    proto, s, _ = witness_cases.case("pb_2s1c_d6")
    r, _ = _bfs(proto, s)
    plain, _ = _bfs(proto, watch_cases.case("pb_2s1c_d6")[1])
    assert _same_search(r, plain) and r.watchCounts() == watch_cases.gold("pb_2s1c_d6")["census"]
    _check_against_fixture("pb_2s1c_d6", r)
    wit = r.watchWitness(0)
    assert wit.depth() == 1 and witness_cases.gold("pb_2s1c_d6")["witnesses"][0]["holders"] == 2
    assert r.watchWitness(1).packed == wit.packed  # the raw-message restatement
    oargs = [a for a in watch_cases.ORACLE_ARGS[("pb_2s1c_d6", 0)] if a not in watch_cases._FIN]
    rep = oracle_util.replay(oargs, wit.trace())
    assert rep["ok"] and rep["depth"] == 1 and rep["goals"][0]["value"]
    want = oracle_util.run("bfs", oargs + LIST, timeout=120)
    assert want["num_terminals"] == 2 and rep["state"] in {t["state"] for t in want["terminals"]}


# ---- 9. refusals and lifetimes through the C ABI ----------------------------------------------------------------------------
def _c_witness(e, w, nb):
    depth, n = ctypes.c_int32(99), ctypes.c_int32(99)
    buf = (ctypes.c_uint8 * nb)()
    rc = e.lib.dsl_watch_witness(e.handle, w, ctypes.byref(depth), None, 0, ctypes.byref(n), buf, nb)
    return rc, depth.value, n.value, bytes(buf)


def test_c_abi_refusals_and_lifetimes():
    proto, s, _ = witness_cases.case("pp_1c10p_extra")
    gold = _gold_packed("pp_1c10p_extra")
    e = Engine(proto)
    try:
        nb = e.state_bytes()
        assert _packed(e.bfs(proto.initial_state(), s), 3) == gold
        assert _c_witness(e, 2, nb) == (0, 20, 20, gold[2]) and _c_witness(e, 0, nb)[:3] == (0, -1, 0)
        # a mask bit at or above the number of watches: refused, named, and the old mask stays
        assert e.lib.dsl_set_watch_witnesses(e.handle, 0b1111) == DSL_ERR_ARG
        assert b"at or above the 3 set" in e.lib.dsl_last_error()
        assert _packed(e.bfs(proto.initial_state(), s), 3) == gold
        # a bad index
        assert _c_witness(e, 3, nb)[0] == DSL_ERR_ARG and _c_witness(e, -1, nb)[0] == DSL_ERR_ARG
        assert b"dsl_watch_witness: watch" in e.lib.dsl_last_error()
        # after a DFS and after a replay there is no witness
        goal = s.clone().addGoal(CLIENTS_DONE)
        g = e.bfs(proto.initial_state(), goal)
        assert g.watchWitness(2).packed == g.goalMatchingState().packed == gold[2]
        d = e.dfs(proto.initial_state(), goal.clone().maxDepth(30), probes=256, max_probes=256, seed=1)
        assert d.watchWitness(2) is None and _c_witness(e, 2, nb)[:3] == (0, -1, 0)
        assert _packed(e.bfs(proto.initial_state(), goal), 3) == gold
        rp = e.replay(proto.initial_state(), goal, g.goalMatchingState().events())
        assert rp.watchWitness(2) is None and _c_witness(e, 2, nb)[:3] == (0, -1, 0)
        # dsl_set_watches resets the mask: the same watches set again want no witness
        _, arr, n, pool, n_pool = s._encode_watches(proto.initial_state())
        assert e.lib.dsl_set_watches(e.handle, arr, n, pool, n_pool) == 0
        res = ctypes.POINTER(_lib.dsl_result)()
        assert e.lib.dsl_run(e.handle, ctypes.byref(res)) == 0
        e.lib.dsl_result_free(res)
        assert [_c_witness(e, w, nb)[1] for w in range(3)] == [-1, -1, -1]
        e._set_witness_mask = 0  # what the engine now holds: the next search asks again
        assert _packed(e.bfs(proto.initial_state(), s), 3) == gold
    finally:
        e.close()


def test_no_witness_request_makes_no_call():
    proto, s, _ = watch_cases.case("pp_1c10p_8w")
    e = Engine(proto)
    try:
        r = e.bfs(proto.initial_state(), s)
        assert getattr(e, "_set_witness_mask", 0) == 0 and [r.watchWitness(i) for i in range(8)] == [None] * 8
        e.bfs(proto.initial_state(), s)  # a repeated search: the engine's buffers have their sizes
        st0 = e.kernel_stats()
        w = e.bfs(proto.initial_state(), witness_cases.with_witnesses(s, which={0}))
        assert e._set_witness_mask == 1 and w.watchWitness(0).depth() == 20 and w.watchWitness(1) is None
        st1 = e.kernel_stats()
        print("host_syncs without / with one witness:", st0["host_syncs"], st1["host_syncs"])
        assert st1["host_syncs"] > st0["host_syncs"]  # the stop and the pass are paid only when asked for
        assert _same_search(r, w) and r.watchCounts() == w.watchCounts()
    finally:
        e.close()
