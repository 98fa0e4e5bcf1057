"""Step invariants on the engine (SearchSettings.addStepInvariant -> k_step_check): every case of
tests/step_cases.py gives what tests/hostcheck/stepcheck.cpp computed on the host with exact state
equality (tests/golden/step.json) -- the end, per_depth, the judged edges per level, the reported
edge byte for byte and its counts -- also from a first table that grows and restarts and with
doErrorChecks, and for a level taken as cut short by the deadline; the reported trace is replayed
and the predicate re-evaluated in Python on every one of its edges; step invariants that hold change nothing of a search, watches, witnesses and the
census included; the priorities within a level; the refusals."""
import ctypes

import pytest

import event_cases
import step_cases
import watch_cases
import witness_cases
from dslabs_amd import (CLIENTS_DONE, RESULTS_OK, EndCondition, Engine, FieldRef, SearchSettings, StatePredicate, _lib,
                        field_value, new, old)
from dslabs_amd import search as S
from dslabs_amd.protocols import PingPong

pytestmark = pytest.mark.gpu
NAMES = sorted(step_cases.CASES)


def _bfs(proto, settings, state=None, engine=None):
    e = engine or Engine(proto)
    try:
        return e.bfs(state if state is not None else proto.initial_state(), settings)
    finally:
        if engine is None:
            e.close()


def _check(r, name, settings):
    g = step_cases.gold(name)
    assert int(r.endCondition()) == g["end"] and r.per_depth == g["per_depth"] and r.initial_depth == g["initial_depth"]
    assert r.stepEdges() == g["edges"]
    term = r.lastState() if g["terminal_depth"] >= 0 else None
    assert (term.depth() if term is not None else -1) == g["terminal_depth"]
    _check_violation(r, g, settings)


def _check_violation(r, g, settings):
    v, gv = r.stepViolation(), g["violation"]
    assert (v is None) == (gv is None)
    if v is None:
        return
    assert (v.index, v.depth, v.edges, v.perInvariant) == (gv["index"], gv["depth"], gv["edges"], gv["per_invariant"])
    assert v.parent.packed.hex() == gv["parent"] and v.state.packed.hex() == gv["state"]
    assert v.parent.depth() == v.depth - 1 and v.state.depth() == v.depth
    assert len(v.state.events()) == v.depth - r.initial_depth and v.state.trace()[:-1] == v.parent.trace()
    assert v.state.trace()[-1] == v.event
    ev, ge = v.state.events()[-1], gv["event"]
    assert (ev.is_timer, ev.from_, ev.to, ev.type) == (ge["is_timer"], ge["from"], ge["to"], ge["type"])
    assert [ev.fields[i] for i in range(ev.n_fields)] == ge["fields"]
    assert v.name == settings.stepInvariants()[v.index].name
    if g["step_terminal"]:  # the step violation is the search's terminal
        assert r.endCondition() == EndCondition.INVARIANT_VIOLATED
        assert r.invariantViolatingState().packed == v.state.packed and r.invariantViolatingState().trace() == v.state.trace()
        assert r.invariantViolated().predicate is settings.stepInvariants()[v.index]
        assert g["pred_index"] == len(settings.invariants()) + v.index


# ---- 1. every case against the host walk ----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_host_walk(name):
    proto, s, state = step_cases.case(name)
    _check(_bfs(proto, s, state), name, s)


@pytest.mark.parametrize("name", ["mp_c5_d8_ir_active", "mp_c5_d8_done", "mp_c5_d8_ir_hold"])
def test_small_first_table_grows_and_restarts_with_the_same_answer(name):
    proto, s, state = step_cases.case(name)
    s.table_log2_slots = 10
    e = Engine(proto)
    try:
        r = e.bfs(proto.initial_state(), s)
        st = e.kernel_stats()
    finally:
        e.close()
    assert st["table_slots"] > (1 << 10) or st["table_rehashes"] > 0  # it grew
    _check(r, name, s)


@pytest.mark.parametrize("name", NAMES)
def test_do_error_checks_gives_the_same_answer(name):
    proto, s, state = step_cases.case(name)
    r = _bfs(proto, s.doErrorChecks(), state)
    assert r.checks["not_deterministic"] == 0
    if len(step_cases.gold(name)["per_depth"]) > 2:  # a level's rows are checked when they become the frontier:
        assert r.checks["run"] > 0                   # a search that ends in its first level checks none
    _check(r, name, s)


def test_violation_of_a_level_the_deadline_cuts_short_is_reported(monkeypatch):
    """DSL_TEST_CUT_DEPTH makes the engine take one level as cut short by max_time_ms: the level is no
    completed depth (no per_depth entry, no edge row), and its step violation is reported whole."""
    name = "mp_c5_d8_ir_active"
    g = step_cases.gold(name)
    proto, s, state = step_cases.case(name)
    monkeypatch.setenv("DSL_TEST_CUT_DEPTH", str(g["violation"]["depth"] - 1))
    r = _bfs(proto, s, state)
    assert r.endCondition() == EndCondition.INVARIANT_VIOLATED
    assert r.per_depth == g["per_depth"][:-1] and r.stepEdges() == g["edges"][:-1]
    assert r.lastState().depth() == g["terminal_depth"]
    _check_violation(r, g, s)
    # the same cut without a violation in the level: the deadline's end, and the rows up to it
    hold, gh = "mp_c5_d8_ir_hold", step_cases.gold("mp_c5_d8_ir_hold")
    proto, s, state = step_cases.case(hold)
    monkeypatch.setenv("DSL_TEST_CUT_DEPTH", "3")
    r = _bfs(proto, s, state)
    assert r.endCondition() == EndCondition.TIME_EXHAUSTED and r.stepViolation() is None
    assert r.per_depth == gh["per_depth"][:4] and r.stepEdges() == gh["edges"][:3]


def test_max_terminals_lists_the_step_terminal_alone():
    proto, s, state = step_cases.case("mp_c5_d8_ir_active")
    r = _bfs(proto, s.maxTerminals(8), state)
    _check(r, "mp_c5_d8_ir_active", s)
    assert r.numTerminals() == 1 and len(r.terminals()) == 1
    end, pred, st = r.terminals()[0]
    assert end == EndCondition.INVARIANT_VIOLATED and pred.predicate is s.stepInvariants()[1]
    assert st.packed == r.stepViolation().state.packed


# ---- 2. the reported trace, independent of the kernel ------------------------------------------------------------
def _py_eval(p, proto, par, succ, event_text, event):
    """A step predicate tree in Python, from field_value / records() of the two states."""
    if p.operands:
        a = _py_eval(p.operands[0], proto, par, succ, event_text, event)
        if p.pred_id == S.PRED_IMPLIES:
            a = not a
        if p.pred_id == S.PRED_AND:
            x = a and _py_eval(p.operands[1], proto, par, succ, event_text, event)
        else:
            x = a or _py_eval(p.operands[1], proto, par, succ, event_text, event)
    elif p.pred_id in (S.PRED_STEP_FIELD, S.PRED_FIELD):
        if p.pred_id == S.PRED_STEP_FIELD:
            desc, cmp, rhs_field, lnew, rnew = S.step_field_arg0_decode(p.arg0)
        else:
            (desc, cmp, rhs_field), lnew, rnew = S.field_arg0_decode(p.arg0), True, True
        ref = lambda d: FieldRef(proto, *S.field_desc_decode(d), "f")  # noqa: E731
        a = field_value(succ if lnew else par, ref(desc))
        b = field_value(succ if rnew else par, ref(p.arg1)) if rhs_field else p.arg1
        x = {S.CMP_EQ: a == b, S.CMP_NE: a != b, S.CMP_LT: a < b, S.CMP_GE: a >= b, S.CMP_LE: a <= b, S.CMP_GT: a > b}[cmp]
    elif p.pred_id == S.PRED_STEP_SENT:
        added = set(succ.records()) - set(par.records())
        x = any(all(c.holds(r) for c in p.conds) for r in added)
    elif p.pred_id == S.PRED_STEP_EVENT:
        names = proto.event_classes()[p.arg0][0].split("|") if p.arg0 >= 0 else None
        x = (names is None or any(f", {n}(" in event_text for n in names)) and (p.arg1 < 0 or event.to == p.arg1)
    else:
        raise NotImplementedError(p.name)
    return (not x) if p.negated else x


def _named(p):
    return any(_named(o) for o in p.operands) if p.operands else \
        p.pred_id not in (S.PRED_STEP_FIELD, S.PRED_FIELD, S.PRED_STEP_SENT, S.PRED_STEP_EVENT)


@pytest.mark.parametrize("name", ["lab0_2c10p_viol", "lab0_2c10p_ir_viol", "kv_test09_ir_viol", "sipaxos_2p3a_d6_viol",
                                  "synth_c3_d3_viol", "mp_c5_d8_slotout", "mp_c5_d8_ir_eight", "mp_c5_d8_ir_heard",
                                  "mp_c5_d8_ir_active", "pb_2s1c_d7_ir_viol", "pb_stage2_viol"])
def test_reported_trace_replays_and_breaks_only_its_last_edge(name):
    proto, s, state = step_cases.case(name)
    start = state if state is not None else proto.initial_state()
    e = Engine(proto)
    try:
        v = e.bfs(start, s).stepViolation()
        events = v.state.events()
        assert len(events) == v.depth - start.depth() >= 1
        states = [start]
        for i in range(1, len(events) + 1):
            rp = e.replay(start, SearchSettings(), events[:i], minimize=False)
            last = rp.lastState()
            assert last is not None and last.depth() == start.depth() + i
            states.append(last)
            assert rp.stepViolation() is None and rp.stepEdges() == []  # a replay judges no step
    finally:
        e.close()
    assert states[-1].packed == v.state.packed and states[-2]._packed_now() == v.parent.packed
    texts = v.state.trace()[-len(events):]
    judged = [(i, p) for i, p in enumerate(s.stepInvariants()) if not _named(p)]
    assert any(i == v.index for i, _ in judged)
    for k in range(len(events)):
        par, succ = states[k], states[k + 1]
        for i, p in judged:
            val = _py_eval(p, proto, par, succ, texts[k], events[k])
            if k < len(events) - 1:
                assert val, (k, p.name)
            elif i == v.index:
                assert not val, p.name
            elif i < v.index:
                assert val, p.name  # the reported index is the lowest violated one


# ---- 3. step invariants that hold change nothing ---------------------------------------------------------------------
def _same_state(engine, start, x, y, replay=True):
    """x and y are the same state at the same depth, each with a trace that leads to it (a state with
    several parents may be traced through either; the levels run one by one with step invariants)."""
    assert x.packed == y.packed and x.depth() == y.depth() and len(x.trace()) == len(y.trace())
    for st in (x, y):
        if st.packed is None or not replay:
            continue
        rp = engine.replay(start if start is not None else st.protocol.initial_state(), SearchSettings(), st.events(),
                           minimize=False)
        assert rp.lastState() is not None and rp.lastState().packed == st.packed


def _goal_case():
    proto, s, state = step_cases.case("prio_goal")
    n = proto.length("client1", "_results")
    return proto, s.clearStepInvariants().addStepInvariant(new(n) >= old(n)), state


@pytest.mark.parametrize("name", ["mp_c5_d8_ir_hold", "pb_stage2_hold", "lab0_2c10p_hold", "goal"])
def test_search_is_the_same_with_and_without(name):
    proto, s, state = _goal_case() if name == "goal" else step_cases.case(name)
    s.maxTerminals(8).addWatch(proto.raw_field(0, 0, 1) == 0, witness=True)
    plain = s.clone().clearStepInvariants()
    e = Engine(proto)
    try:
        a = _bfs(proto, plain, state, e)
        b = _bfs(proto, s, state, e)
        c = _bfs(proto, plain, state, e)  # and off again on the same engine
        assert a.stepEdges() == [] and c.stepEdges() == [] and len(b.stepEdges()) >= 1
        assert a.stepViolation() is None and b.stepViolation() is None and c.stepViolation() is None
        if name != "goal":
            assert b.stepEdges() == step_cases.gold(name)["edges"]
        for r in (b, c):
            assert (r.states, r.per_depth, r.successors) == (a.states, a.per_depth, a.successors)
            assert r.endCondition() == a.endCondition()
            assert r.numTerminals() == a.numTerminals() and len(r.terminals()) == len(a.terminals())
            for (e1, p1, s1), (e2, p2, s2) in zip(r.terminals(), a.terminals()):
                assert e1 == e2 and (p1 is None) == (p2 is None)
                _same_state(e, state, s1, s2)
            ta, tr = a.lastState(), r.lastState()
            assert (ta is None) == (tr is None)
            if ta is not None:
                _same_state(e, state, tr, ta)
            assert r.watchCounts() == a.watchCounts() and r.watchTotal(0) == a.watchTotal(0)
            wa, wr = a.watchWitness(0), r.watchWitness(0)
            assert (wa is None) == (wr is None)
            if wa is not None:
                _same_state(e, state, wr, wa)
        if name == "goal":
            assert a.endCondition() == EndCondition.GOAL_FOUND and a.goalMatchingState() is not None
    finally:
        e.close()


def test_watches_two_witnesses_and_the_census_keep_their_goldens():
    """Everything on at once: each output equals its own golden."""
    name = "mpir_c5_d8_generic"
    proto, s, _ = watch_cases.case(name)
    s = witness_cases.with_witnesses(s, which={0, 3}).eventCensus()
    step_cases.CASES["mp_c5_d8_ir_hold"][1](proto, s)
    r = _bfs(proto, s)
    gw, gc, gs = watch_cases.gold(name), event_cases.gold("mp_c5_d8_ir"), step_cases.gold("mp_c5_d8_ir_hold")
    assert r.per_depth == gw["per_depth"] == gs["per_depth"] and r.endCondition() == EndCondition.SPACE_EXHAUSTED
    assert r.watchCounts() == gw["census"]
    for w in range(8):
        want = witness_cases.gold_state(name, w) if w in (0, 3) else None
        got = r.watchWitness(w)
        assert (got.packed if got is not None else None) == want
    assert r.eventRows() == [event_cases.dense(row, gc["classes"], gc["nodes"]) for row in gc["rows"]]
    assert r.stepEdges() == gs["edges"] and r.stepViolation() is None
    # and with a violated one: the census has a row for the violating level, the watches their counts up to it
    s2 = s.clone().clearStepInvariants()
    step_cases.CASES["mp_c5_d8_ir_active"][1](proto, s2)
    r2 = _bfs(proto, s2)
    ga = step_cases.gold("mp_c5_d8_ir_active")
    assert r2.per_depth == ga["per_depth"] and r2.stepEdges() == ga["edges"] and r2.stepViolation().depth == 7
    assert r2.eventRows() == r.eventRows()[:7] and r2.watchCounts() == [c[:8] for c in gw["census"]]


# ---- 4. priority within the violating level ---------------------------------------------------------------------------
def test_state_invariant_outranks_and_the_step_violation_is_still_there():
    proto, s, state = step_cases.case("prio_inv")
    r = _bfs(proto, s, state)
    _check(r, "prio_inv", s)
    assert r.endCondition() == EndCondition.INVARIANT_VIOLATED
    assert r.invariantViolated().predicate is s.invariants()[-1]  # the state invariant, reported as without step invariants
    plain = _bfs(proto, s.clone().clearStepInvariants(), state)
    assert plain.invariantViolatingState().packed == r.invariantViolatingState().packed
    v = r.stepViolation()
    assert v is not None and v.index == 0 and v.depth == r.invariantViolatingState().depth()


def test_goal_of_the_same_level_loses_to_the_step_violation():
    proto, s, state = step_cases.case("prio_goal")
    r = _bfs(proto, s, state)
    _check(r, "prio_goal", s)
    assert r.endCondition() == EndCondition.INVARIANT_VIOLATED and r.goalMatchingState() is None
    plain = _bfs(proto, s.clone().clearStepInvariants(), state)
    assert plain.endCondition() == EndCondition.GOAL_FOUND and plain.goalMatchingState().depth() == r.stepViolation().depth
    assert plain.per_depth == r.per_depth


def test_exception_of_the_same_level_is_reported():
    proto, s, state = step_cases.case("minitest_viol")
    r = _bfs(proto, s, state)
    _check(r, "minitest_viol", s)
    assert r.endCondition() == EndCondition.EXCEPTION_THROWN and r.exceptionalState() is not None
    assert r.stepViolation() is not None and r.stepViolation().depth == 2 and r.stepEdges() == [1, 1]


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def _set_steps(e, settings, proto):
    enc = settings._encode_steps(proto.initial_state())
    return e.lib.dsl_set_step_invariants(e.handle, enc[1], enc[2], enc[3], enc[4])


def test_engine_refusals_keep_what_it_had():
    proto = PingPong(1, 10)
    nres = proto.raw_field("client1", 8, 4)
    step = new(nres) >= old(nres)
    m = proto.raw_message("PongReply", 32)
    raw = lambda pid, a0=0, a1=0: StatePredicate("raw", pid, a0, a1)  # noqa: E731
    good = SearchSettings().addInvariant(RESULTS_OK).addPrune(CLIENTS_DONE).addStepInvariant(step)
    gold = step_cases.gold("lab0_1c10p_hold")
    e = Engine(proto)
    try:
        r0 = e.bfs(proto.initial_state(), good)
        assert r0.per_depth == gold["per_depth"] and r0.stepEdges() == gold["edges"]

        def refused(text, settings=None, rc=-1):
            if settings is not None:
                assert _set_steps(e, settings, proto) == rc
            assert text in e.lib.dsl_last_error().decode(), e.lib.dsl_last_error()
            # the engine keeps what it had: the same search, the same rows
            e._set_enc = None
            r = e.bfs(proto.initial_state(), good)
            assert r.per_depth == gold["per_depth"] and r.stepEdges() == gold["edges"]

        # nine step invariants
        arr = (_lib.dsl_predicate * 9)(*[step._encode(proto.initial_state(), []) for _ in range(9)])
        assert e.lib.dsl_set_step_invariants(e.handle, ctypes.cast(arr, ctypes.POINTER(_lib.dsl_predicate)), 9, None, 0) == -1
        refused("step invariants: 9, outside 0..8")
        # DSL_PRED_NET in a step tree
        s = SearchSettings()
        s._step_invariants.append(step.or_(m.where(m.raw_field(31, 1) == 1)))
        refused("DSL_PRED_NET in a step invariant is not supported", s)
        # a descriptor past the node, a class out of range
        refused("beyond the node's 160 bits", SearchSettings().addStepInvariant(
            raw(S.PRED_STEP_FIELD, S.step_field_arg0(S.field_desc(1, 5 * 32, 8), S.CMP_EQ, False, True, False), 0)))
        refused("class 3 outside the protocol's 3 handler classes", SearchSettings().addStepInvariant(raw(S.PRED_STEP_EVENT, 3, -1)))
        # a step leaf in each of the four other lists
        for lst, word in (("_invariants", "invariants"), ("_goals", "goals"), ("_prunes", "prunes")):
            bad = SearchSettings()
            getattr(bad, lst).append(step)
            enc = bad._encode(proto.initial_state())
            assert e.lib.dsl_set_settings(e.handle, ctypes.byref(enc)) == -1
            refused(f"step leaf DSL_PRED_STEP_FIELD in the {word}")
        bad = SearchSettings()
        bad._watches.append(proto.delivered("PongReply"))
        bad._witness.append(False)
        w = bad._encode_watches(proto.initial_state())
        assert e.lib.dsl_set_watches(e.handle, w[1], w[2], w[3], w[4]) == -1
        refused("step leaf DSL_PRED_STEP_EVENT in the watches")
        # a budget overflow in either call order: 1 + 4 x 11 program steps in the settings, 2 x 11 here
        big, sbig = nres >= 0, step
        for _ in range(5):
            big, sbig = big.and_(nres >= 0), sbig.and_(step)
        heavy = SearchSettings().addInvariant(RESULTS_OK).addPrune(CLIENTS_DONE)
        for _ in range(4):
            heavy.addInvariant(big)
        two = SearchSettings().addStepInvariant(sbig).addStepInvariant(sbig)
        assert _set_steps(e, two, proto) == 0  # the steps first (2 + 22 ops) ...
        henc = heavy._encode(proto.initial_state())
        assert e.lib.dsl_set_settings(e.handle, ctypes.byref(henc)) == -1  # ... then the settings overflow the sum
        assert "predicate programs too long" in e.lib.dsl_last_error().decode()
        assert _set_steps(e, SearchSettings(), proto) == 0 and e.lib.dsl_set_settings(e.handle, ctypes.byref(henc)) == 0
        assert _set_steps(e, two, proto) == -1  # the settings first: now the steps are the ones refused
        assert "predicate programs too long" in e.lib.dsl_last_error().decode()
        # ... and the engine kept the heavy settings without step invariants
        res_p = ctypes.POINTER(_lib.dsl_result)()
        assert e.lib.dsl_run(e.handle, ctypes.byref(res_p)) == 0
        assert [res_p.contents.per_depth[i] for i in range(res_p.contents.n_levels)] == gold["per_depth"]
        e.lib.dsl_result_free(res_p)
        n = ctypes.c_int32(-1)
        assert e.lib.dsl_step_edges(e.handle, None, 0, ctypes.byref(n), None) == 0 and n.value == 0
    finally:
        e.close()


def test_step_invariants_are_refused_on_several_shards():
    proto, s, _ = step_cases.case("mp_c5_d8_hold")
    e = Engine(proto, virtual_shards=3, replicate_below=0)
    try:
        with pytest.raises(_lib.EngineError) as err:
            e.bfs(proto.initial_state(), s)
        assert err.value.code == -1 and "dsl_run" in str(err.value)
        assert "step invariants are not supported in a search over more than one shard" in str(err.value)
        r = e.bfs(proto.initial_state(), s.clone().clearStepInvariants())  # the same engine, without them
        assert r.per_depth == step_cases.gold("mp_c5_d8_hold")["per_depth"] and r.stepEdges() == []
    finally:
        e.close()


def test_a_search_over_several_processes_refuses_before_any_collective():
    from dslabs_amd import distributed as d
    calls = []

    def cb(*_):
        calls.append(1)
        return 1

    class Comm:
        cbs = (d.ALLGATHER(cb), d.ALLREDUCE(cb), d.BCAST(cb), d.ALLTOALLV(cb))
        struct = d.dsl_host_comm(None, 0, 2, *cbs, 0, 0)

    proto = PingPong(1, 2)
    nres = proto.raw_field("client1", 8, 4)
    e = Engine(proto, rank=0, world_size=2, host_comm=Comm())
    try:
        with pytest.raises(_lib.EngineError) as err:
            e.bfs(proto.initial_state(), SearchSettings().addStepInvariant(new(nres) >= old(nres)))
        assert err.value.code == -1 and "step invariants are not supported" in str(err.value)
        assert calls == []
    finally:
        e.close()


def test_dfs_and_replay_report_no_step_data_and_plain_searches_make_no_new_call():
    proto, s, _ = step_cases.case("lab0_1c10p_ir_viol")
    e = Engine(proto)
    try:
        idx = ctypes.c_int32(7)
        assert e.lib.dsl_step_violation(e.handle, ctypes.byref(idx), None, None, None, None, 0, None, None, None, 0) == 0
        assert idx.value == -1  # before any search
        r = e.bfs(proto.initial_state(), s)
        _check(r, "lab0_1c10p_ir_viol", s)
        assert e.lib.dsl_step_violation(e.handle, ctypes.byref(idx), None, None, None, None, 0, None, None, None, 0) == 0
        assert idx.value == 1
        goal = s.clone().addGoal(CLIENTS_DONE).maxDepth(30)
        d = e.dfs(proto.initial_state(), goal, probes=256, max_probes=256, seed=1)
        assert d.stepEdges() == [] and d.stepViolation() is None
        assert d.endCondition() in (EndCondition.GOAL_FOUND, EndCondition.TIME_EXHAUSTED)  # a DFS judges no step
        assert e.lib.dsl_step_violation(e.handle, ctypes.byref(idx), None, None, None, None, 0, None, None, None, 0) == 0
        assert idx.value == -1
        rp = e.replay(proto.initial_state(), s, r.stepViolation().state.events())
        assert rp.endCondition() == EndCondition.SPACE_EXHAUSTED and rp.stepViolation() is None and rp.stepEdges() == []
    finally:
        e.close()
    e2 = Engine(proto)
    try:
        plain = e2.bfs(proto.initial_state(), s.clone().clearStepInvariants())
        assert plain.stepEdges() == [] and plain.stepViolation() is None and not hasattr(e2, "_set_step_key")
    finally:
        e2.close()
