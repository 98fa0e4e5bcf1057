"""Step invariants (SearchSettings.addStepInvariant -> dsl_set_step_invariants), the parts that need
no GPU: the host truth of every case (tests/hostcheck/stepcheck.cpp: a breadth-first walk with exact
state equality that evaluates every step invariant twice on every judged edge, also built with
-fsanitize=undefined and run directly) compared with the committed tests/golden/step.json, tied to
the oracle's committed per_depth and to the committed event census (edges judged = events - noops -
exceptions, level by level); the conditions the cases were chosen for; the Python encoding against
the header's macros; the refusals that need no engine; the three entry points against the C header."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import pytest

import event_cases
import step_cases
from dslabs_amd import CLIENTS_DONE, RESULTS_OK, SearchSettings, StatePredicate, _lib, new, old
from dslabs_amd import search as S
from dslabs_amd.protocols import MultiPaxosIR, PingPong, PingPongIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
NAMES = sorted(step_cases.CASES)
ANCHORED = [n for n in NAMES if n not in step_cases.STARTS]  # the cases that start where their event case does


# ---- 1. the host truth ------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "ubsan"])
def rows(request, lib):
    exe = step_cases.stepcheck_build(request.param)
    return {name: step_cases.stepcheck_run(exe, name) for name in step_cases.CASES}


@pytest.mark.parametrize("name", NAMES)
def test_walk_reproduces_the_fixture(rows, name):
    row, gold = rows[name], step_cases.gold(name)
    assert row["errors"] == 0 and row["mismatches"] == 0  # eval_step_prog against the plain evaluation
    for k in gold:
        assert row[k] == gold[k], k


def test_fixture_has_every_case_and_no_other():
    assert sorted(step_cases.gold()) == NAMES


@pytest.mark.parametrize("name", ANCHORED)
def test_per_depth_is_the_oracles(name):
    """A search with step invariants that hold is the plain search; one that is violated is its
    prefix up to the violating level (which is completed)."""
    g, base = step_cases.gold(name), step_cases.CASES[name][0]
    want = event_cases.fixture_per_depth(base)
    if want is None or name.startswith("prio_"):  # no oracle fixture; the priority cases add a state predicate
        want = event_cases.gold(base)["per_depth"]
        if name.startswith("prio_"):
            assert g["per_depth"] == want[:len(g["per_depth"])]
            return
    if g["violation"] is None:
        assert g["per_depth"] == want
    else:
        assert g["per_depth"] == want[:len(g["per_depth"])]
        assert len(g["per_depth"]) - 1 == g["violation"]["depth"] - g["initial_depth"]


@pytest.mark.parametrize("name", ANCHORED)
def test_edges_are_the_census_events_that_changed_something(name):
    """edges[i] = the sum over row i's cells of events - noops - exceptions, up to the violating level."""
    g, cen = step_cases.gold(name), event_cases.gold(step_cases.CASES[name][0])
    want = [sum(c[2] - c[3] - c[4] for c in row) for row in cen["rows"]]
    assert g["edges"] == want[:len(g["edges"])] and len(g["edges"]) >= 1
    if g["violation"] is None:
        assert len(g["edges"]) == len(want)


@pytest.mark.parametrize("name", [n for n in ANCHORED if step_cases.CASES[n][2] == "hold"])
def test_holding_cases_end_as_the_plain_search(name):
    g, cen = step_cases.gold(name), event_cases.gold(step_cases.CASES[name][0])
    assert g["violation"] is None and not g["step_terminal"] and g["pred_index"] == -1
    assert g["end"] == 3 and cen["end"] == 0  # DSL_SPACE_EXHAUSTED; the census fixture's verdict: none
    assert g["per_depth"] == cen["per_depth"]


@pytest.mark.parametrize("form", ["pb_dropped", "pb_dropped_ir"])
def test_dropped_only_cases_are_decided_by_the_dropped_set(lib, form):
    """The named network leaves of these cases are true through dropped records alone: from the same
    start without its dropped set, the holding case is violated by the first level."""
    from dslabs_amd.search import SearchState
    exe = step_cases.stepcheck_build("plain")
    proto, _, st = step_cases.case(form + "_hold")
    assert st.droppedMessages()
    g, gv = step_cases.gold(form + "_hold"), step_cases.gold(form + "_viol")
    assert g["violation"] is None and g["end"] == 3 and len(g["edges"]) >= 2 and min(g["edges"]) > 0
    assert gv["violation"]["index"] == 1 and gv["violation"]["depth"] == st.depth() + 1
    assert gv["violation"]["edges"] == gv["edges"][0] == g["edges"][0]  # every edge of the first level
    bare = SearchState(proto, st._packed_now(), st.depth())
    assert not bare.droppedMessages()
    row = step_cases.stepcheck_run(exe, form + "_hold", start=bare)
    assert row["violation"] is not None and row["violation"]["index"] == 0 and row["violation"]["depth"] == st.depth() + 1


def test_the_conditions_the_cases_were_chosen_for():
    import make_step_golden
    make_step_golden.check_conditions(step_cases.gold())
    g = step_cases.gold()
    # the reported terminal of a step violation: depth(P) + 1 and the index past the state invariants
    v = g["mp_c5_d8_ir_slotout"]
    assert v["step_terminal"] and v["end"] == 1 and v["pred_index"] == 3 + 1 and v["terminal_depth"] == v["violation"]["depth"]
    # the large frontiers: 1,561 and 4,050 parents
    assert g["mp_c5_d8_ir_active"]["per_depth"][6] == 1561 and g["mp_c5_d8_done"]["per_depth"][7] == 4050
    assert g["mp_c5_d8_done"]["violation"]["depth"] == 8 and g["mp_c5_d8_done"]["violation"]["edges"] == 16
    # a staged start: the violation's depth is absolute
    assert g["pb_stage2_viol"]["initial_depth"] == 11 and g["pb_stage2_viol"]["violation"]["depth"] == 12
    # the hand-written and the generated form of one protocol agree
    for a, b in (("lab0_1c10p_viol", "lab0_1c10p_ir_viol"), ("lab0_2c10p_hold", "lab0_2c10p_ir_hold"),
                 ("mp_c5_d8_hold", "mp_c5_d8_ir_hold")):
        assert (g[a]["per_depth"], g[a]["edges"], g[a]["end"]) == (g[b]["per_depth"], g[b]["edges"], g[b]["end"])
    a, b = g["mp_c5_d8_slotout"]["violation"], g["mp_c5_d8_ir_slotout"]["violation"]
    ev = lambda e: (e["k"], e["is_timer"], e["from"], e["to"], e["type"])  # noqa: E731 (the two forms pack the fields differently)
    assert (a["depth"], a["edges"], a["per_invariant"], ev(a["event"])) == (b["depth"], b["edges"], b["per_invariant"], ev(b["event"]))


# ---- 2. the Python encoding against the header's macros ----------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "dslabs_hip.h")) as f:
        return f.read()


def test_ids_and_bits_are_the_headers():
    hdr = _header()
    for name, val in (("DSL_PRED_STEP_FIELD", S.PRED_STEP_FIELD), ("DSL_PRED_STEP_SENT", S.PRED_STEP_SENT),
                      ("DSL_PRED_STEP_EVENT", S.PRED_STEP_EVENT)):
        assert int(re.search(name + r" = (\d+)", hdr).group(1)) == val
    assert (S.PRED_STEP_FIELD, S.PRED_STEP_SENT, S.PRED_STEP_EVENT) == (953, 954, 955)
    assert int(re.search(r"#define DSL_STEP_LHS_NEW_BIT (\d+)", hdr).group(1)) == S.STEP_LHS_NEW_BIT == 36
    assert int(re.search(r"#define DSL_STEP_RHS_NEW_BIT (\d+)", hdr).group(1)) == S.STEP_RHS_NEW_BIT == 37
    assert int(re.search(r"#define DSL_MAX_STEP_INVARIANTS (\d+)", hdr).group(1)) == _lib.DSL_MAX_STEP_INVARIANTS == 8


def test_macros_round_trip_through_a_c_compiler(tmp_path):
    """DSL_STEP_FIELD_ARG0 and its decoders, compiled from the header, give what search.py encodes."""
    mp = MultiPaxosIR(3, 2, "append-xy")
    a, b = mp.field("server2", "round"), mp.field("server1", "log", 1).bits(0, 2)
    preds = [new(a) >= old(a), old(b) == 2, new(a) < new(b), old(a) != new(b), new(b) <= 3]
    src = ['#include "dslabs_hip.h"', "#include <stdio.h>", "int main(void) {"]
    for p in preds:
        d, cmp, rf, ln, rn = S.step_field_arg0_decode(p.arg0)
        src.append(f'  printf("%lld %u %d %d %d %d\\n", (long long)DSL_STEP_FIELD_ARG0({d}u, {cmp}, {int(rf)}, {int(ln)}, {int(rn)}), '
                   f"DSL_FIELD_ARG0_DESC({p.arg0}ll), DSL_FIELD_ARG0_CMP({p.arg0}ll), DSL_FIELD_ARG0_RHS_IS_FIELD({p.arg0}ll), "
                   f"DSL_STEP_ARG0_LHS_NEW({p.arg0}ll), DSL_STEP_ARG0_RHS_NEW({p.arg0}ll));")
    src += ["  return 0;", "}"]
    c = tmp_path / "m.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "m"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    for p, line in zip(preds, out):
        d, cmp, rf, ln, rn = S.step_field_arg0_decode(p.arg0)
        assert [int(x) for x in line.split()] == [p.arg0, d, cmp, int(rf), int(ln), int(rn)]
    assert [S.step_field_arg0_decode(p.arg0)[2:] for p in preds] == \
        [(True, True, False), (False, False, False), (True, True, True), (True, False, True), (False, True, False)]
    assert preds[0].arg1 == a.desc() and preds[1].arg1 == 2 and preds[0].name == "new(server2.round) >= old(server2.round)"


def test_sent_and_delivered_encode_as_the_header_says():
    mp = MultiPaxosIR(3, 2, "append-xy")
    st = mp.initial_state()
    d = mp.message("Decision", frm="server2")
    sent = d.sent(d.field("slot") == 1)
    where = d.where(d.field("slot") == 1)
    pool = []
    enc = sent._encode(st, pool)
    assert sent.pred_id == S.PRED_STEP_SENT and sent.name.startswith("sent Decision")
    key = lambda c: (c.bit, c.width, c.cmp, c.const)  # noqa: E731
    assert [key(c) for c in sent.conds] == [key(c) for c in where.conds] and len(sent.conds) == 3  # type, from, slot
    assert (enc.pred_id, enc.negate, enc.arg0, enc.arg1) == (954, 0, 0, len(sent.conds)) and len(pool) == len(sent.conds)
    assert all(q.pred_id == S.PRED_REC_COND for q in pool)
    classes = [n for n, _ in mp.event_classes()]
    ev = mp.delivered("P2a", to="server3")
    assert (ev.pred_id, ev.arg0, ev.arg1) == (955, classes.index("P2a"), 2) and ev.name == "delivered P2a to server3"
    anyev = mp.delivered()
    assert (anyev.arg0, anyev.arg1) == (-1, -1)
    assert mp.delivered(cls=classes.index("Decision")).arg0 == classes.index("Decision")
    e2 = ev.negate()._encode(st, [])
    assert (e2.pred_id, e2.negate, e2.arg0, e2.arg1) == (955, 1, classes.index("P2a"), 2)


def test_settings_keep_step_invariants_apart_from_dsl_settings():
    p = PingPongIR(1, 10)
    st = p.initial_state()
    n = p.length("client1", "_results")
    s = SearchSettings().addInvariant(RESULTS_OK)
    enc0 = bytes(s._encode(st))
    assert s._encode_steps(st) == S._NO_WATCHES
    inv = S.statePredicate("results only grow", new(n) >= old(n))
    assert s.addStepInvariant(inv) is s and s.stepInvariants() == [inv] and inv.name == "results only grow"
    assert bytes(s._encode(st)) == enc0  # dsl_settings carries no step invariant: byte-identical
    key, arr, cnt, pool, n_pool = s._encode_steps(st)
    assert cnt == 1 and n_pool == 0 and arr[0].pred_id == 953 and s._encode_steps(st)[1] is arr  # cached
    c = s.clone()
    assert c.stepInvariants() == [inv] and c.clearStepInvariants() is c and c.stepInvariants() == [] and s.stepInvariants() == [inv]
    s.addStepInvariant((new(n) >= old(n)).and_(p.delivered("PongReply")))
    assert s._encode_steps(st)[0] != key and s._encode_steps(st)[4] == 2


def test_results_without_step_invariants():
    r = S.SearchResults(S.EndCondition.SPACE_EXHAUSTED, 3, [1, 2], 4, 5, None, None, 0.1, 2)
    assert r.stepEdges() == [] and r.stepViolation() is None


# ---- 3. the refusals that need no engine ------------------------------------------------------------------------------
def test_python_refusals():
    p = PingPongIR(1, 10)
    n = p.length("client1", "_results")
    step = new(n) >= old(n)
    s = SearchSettings()
    for add in (s.addInvariant, s.addGoal, s.addPrune, s.addWatch):
        for leaf in (step, p.message("PongReply").sent(), p.delivered("PongReply"), RESULTS_OK.and_(step)):
            with pytest.raises(ValueError, match="is a step leaf"):
                add(leaf)
    assert s.invariants() == [] and s.goals() == [] and s.prunes() == [] and s.watches() == []
    with pytest.raises(ValueError, match=r"use \.sent"):
        s.addStepInvariant(step.or_(p.message("PongReply").where()))
    for k in range(8):
        s.addStepInvariant(step)
    with pytest.raises(ValueError, match="too many step invariants: at most 8"):
        s.addStepInvariant(step)
    # a bare FieldRef on either side says to wrap it
    for bad in (lambda: new(n) >= n, lambda: n >= old(n), lambda: old(n) == p.field("client1", "ping")):
        with pytest.raises(TypeError, match=r"wrap .* in old\(\.\.\.\) or new\(\.\.\.\)|old\(\.\.\.\) or new\(\.\.\.\)"):
            bad()
    with pytest.raises(TypeError):
        new(3)
    with pytest.raises(TypeError):
        new(n) >= "x"
    with pytest.raises(ValueError, match="32 unsigned bits"):
        new(n) >= 1 << 32
    with pytest.raises(ValueError, match="different protocol objects"):
        new(n) >= old(PingPongIR(1, 10).length("client1", "_results"))
    with pytest.raises(ValueError, match="unknown handler class"):
        p.delivered("NoSuchMessage")
    with pytest.raises(ValueError, match="unknown handler class"):
        p.delivered(cls=17)
    with pytest.raises(ValueError, match="unknown address"):
        p.delivered(to="nobody")
    with pytest.raises(ValueError, match="outside"):
        new(n).bits(3, 9)


def _blob_file(proto, settings, d):
    path = os.path.join(str(d), "case.blob")
    with open(path, "wb") as f:
        f.write(step_cases.blob(proto, settings))
    return path


def _refused(proto, settings):
    """stepcheck's answer to settings the engine's own compiler (resolve_settings, check_step_leaves)
    refuses: its text."""
    exe = step_cases.stepcheck_build("plain")
    with tempfile.NamedTemporaryFile("wb", suffix=".blob", delete=False) as f:
        f.write(step_cases.blob(proto, settings))
        path = f.name
    try:
        r = subprocess.run([exe, "refusal", path], capture_output=True, text=True, timeout=60)
    finally:
        os.unlink(path)
    assert r.returncode == 1 and r.stderr.startswith("settings refused: "), r.stdout + r.stderr
    return r.stderr


def test_the_settings_compiler_refuses(lib, tmp_path):
    p = PingPong(1, 10)
    nres = p.raw_field("client1", 8, 4)
    step = new(nres) >= old(nres)
    m = p.raw_message("PongReply", 32)
    raw = lambda pid, a0=0, a1=0: StatePredicate("raw", pid, a0, a1)  # noqa: E731
    base = lambda: SearchSettings().addInvariant(RESULTS_OK)  # noqa: E731
    # a step leaf in each of the three lists of dsl_settings names the leaf and the list
    for lst, word in (("_invariants", "invariants"), ("_goals", "goals"), ("_prunes", "prunes")):
        for leaf, lname in ((step, "DSL_PRED_STEP_FIELD"), (m.sent(m.raw_field(31, 1) == 1), "DSL_PRED_STEP_SENT"),
                            (p.delivered("PongReply"), "DSL_PRED_STEP_EVENT")):
            s = base()
            getattr(s, lst).append(leaf)
            assert f"step leaf {lname} in the {word}" in _refused(p, s)
    # DSL_PRED_NET in a step tree
    s = base()
    s._step_invariants.append(step.or_(m.where(m.raw_field(31, 1) == 1)))
    assert "DSL_PRED_NET in a step invariant is not supported" in _refused(p, s)
    # a descriptor past the node, a record condition past the record, a class out of range, a bad node
    s = base().addStepInvariant(raw(S.PRED_STEP_FIELD, S.step_field_arg0(S.field_desc(1, 5 * 32, 8), S.CMP_EQ, False, True, False), 0))
    assert "beyond the node's 160 bits" in _refused(p, s)
    s = base().addStepInvariant(raw(S.PRED_STEP_FIELD, S.step_field_arg0(S.field_desc(7, 0, 8), S.CMP_EQ, False, True, False), 0))
    assert "node index >= the protocol's 2 nodes" in _refused(p, s)
    s = base().addStepInvariant(raw(S.PRED_STEP_FIELD, S.field_arg0(S.field_desc(1, 0, 8), S.CMP_EQ, False) | 1 << 37, 0))
    assert "bit 37" in _refused(p, s)
    s = base().addStepInvariant(raw(S.PRED_STEP_FIELD, S.field_arg0(S.field_desc(1, 0, 8), S.CMP_EQ, False) | 1 << 38, 0))
    assert "arg0 has bits set above" in _refused(p, s)
    s = base().addStepInvariant(StatePredicate("wide", S.PRED_STEP_SENT, conds=(S.RecCond(30, 8, S.CMP_EQ, 1, "x"),)))
    assert "beyond the record's 32 bits" in _refused(p, s)
    s = base().addStepInvariant(raw(S.PRED_STEP_EVENT, 3, -1))
    assert "class 3 outside the protocol's 3 handler classes" in _refused(p, s)
    s = base().addStepInvariant(raw(S.PRED_STEP_EVENT, -2, -1))
    assert "step event leaf: class -2" in _refused(p, s)
    s = base().addStepInvariant(raw(S.PRED_STEP_EVENT, -1, 2))
    assert "step event leaf: node 2" in _refused(p, s)
    # the shared budget: 64 program steps in all
    # (with the settings' own programs: 1 + 4 x 11 ops there, 2 x 11 here)
    s = base()
    big, sbig = nres >= 0, step
    for _ in range(5):
        big, sbig = big.and_(nres >= 0), sbig.and_(step)
    for _ in range(4):
        s.addInvariant(big)
    s.addStepInvariant(sbig)  # 56 ops: accepted
    assert subprocess.run([step_cases.stepcheck_build("plain"), "fits", _blob_file(p, s.clone().maxDepth(2), tmp_path)],
                          capture_output=True, text=True).returncode == 0
    s.addStepInvariant(sbig)  # 67 ops
    assert "predicate programs too long" in _refused(p, s)
    # a protocol's named leaf of another protocol
    s = base().addStepInvariant(raw(400))
    assert "predicate not supported" in _refused(p, s)
    # and what is legal is accepted: a named leaf and DSL_PRED_FIELD inside a step tree
    ok = base().addStepInvariant(CLIENTS_DONE.negate().or_(step).or_(nres >= 1))
    exe = step_cases.stepcheck_build("plain")
    with tempfile.NamedTemporaryFile("wb", suffix=".blob", delete=False) as f:
        f.write(step_cases.blob(p, ok.maxDepth(3)))
    try:
        assert subprocess.run([exe, "ok", f.name], capture_output=True, text=True).returncode == 0
    finally:
        os.unlink(f.name)


# ---- 4. the C ABI: three more entry points, still ABI 6 ----------------------------------------------------------------
def test_header_declares_the_entry_points_and_abi_stays_6():
    hdr = _header()
    assert int(re.search(r"#define DSL_ABI_VERSION (\d+)", hdr).group(1)) == 6 == _lib.DSL_ABI_VERSION
    flat = re.sub(r"\s+", " ", hdr)
    for decl in ("int dsl_set_step_invariants(dsl_engine* e, const dsl_predicate* preds, int32_t n, const dsl_predicate* pool, "
                 "int32_t n_pool);",
                 "int dsl_step_edges(dsl_engine* e, uint64_t* per_level, int32_t cap, int32_t* n_levels, uint64_t* total);",
                 "int dsl_step_violation(dsl_engine* e, int32_t* index, int32_t* depth, uint64_t* edges_violating, "
                 "uint64_t per_invariant[DSL_MAX_STEP_INVARIANTS], dsl_event* trace, int32_t cap, int32_t* trace_len, "
                 "uint8_t* parent_state, uint8_t* state, size_t len);"):
        assert decl in flat, decl
    assert "Still 6 with dsl_set_step_invariants / dsl_step_edges / dsl_step_violation" in flat
    assert "step invariants" in flat and "is NOT added" in flat  # the set semantics of "added" are stated
    assert {"dsl_set_step_invariants", "dsl_step_edges", "dsl_step_violation"} <= set(_lib.EXPORTED)
    import dslabs_amd
    assert {"old", "new", "StepViolation"} <= set(dslabs_amd.__all__)


def test_ctypes_prototypes_and_null_engine_refusals(lib):
    P = ctypes.POINTER
    assert lib.dsl_set_step_invariants.argtypes == [ctypes.c_void_p, P(_lib.dsl_predicate), ctypes.c_int32,
                                                    P(_lib.dsl_predicate), ctypes.c_int32]
    assert lib.dsl_set_step_invariants(None, None, 0, None, 0) == -1
    assert b"dsl_set_step_invariants" in lib.dsl_last_error()
    n, tot = ctypes.c_int32(7), ctypes.c_uint64(7)
    assert lib.dsl_step_edges(None, None, 0, ctypes.byref(n), ctypes.byref(tot)) == -1 and n.value == 0 and tot.value == 0
    idx, dep = ctypes.c_int32(5), ctypes.c_int32(5)
    assert lib.dsl_step_violation(None, ctypes.byref(idx), ctypes.byref(dep), None, None, None, 0, None, None, None, 0) == -1
    assert idx.value == -1 and dep.value == -1
