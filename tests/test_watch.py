"""Watches (SearchSettings.addWatch -> dsl_set_watches / dsl_watch_counts), the parts that need no
GPU: the Python encoding and its limits, the two entry points' prototypes against the C header, the
host's refusals and the kept `flat` (resolve_settings through tests/hostcheck/watchcheck.cpp), the
host census of every watched search (watchcheck: two independent evaluations per discovered state,
also built with -fsanitize=undefined) against the committed tests/golden/watch.json, and the
oracle's goal searches as the anchor of the named watches' truth."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import oracle_util
import watch_cases
from dslabs_amd import CLIENTS_DONE, NONE_DECIDED, RESULTS_OK, SearchSettings, _lib
from dslabs_amd import search as S
from dslabs_amd.protocols import MultiPaxos, MultiPaxosIR, PingPongIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "dslabs_hip.h")) as f:
        return f.read()


# ---- 1. encoding ---------------------------------------------------------------------------------------
def test_add_watch_clone_and_signature():
    p = PingPongIR(1, 10)
    st = p.initial_state()
    s = SearchSettings().addInvariant(RESULTS_OK)
    assert s.watches() == [] and s._encode_watches(st) == (b"", None, 0, None, 0)
    sig0, enc0 = s._signature(st), s._encode(st)
    done = p.length("client1", "_results") == 10
    assert s.addWatch(CLIENTS_DONE).addWatch(done) is s
    assert s.watches() == [CLIENTS_DONE, done]
    assert s._signature(st) != sig0  # the watches are part of what a search is
    c = s.clone()
    assert c.watches() == s.watches() and c._signature(st) == s._signature(st)
    c.addWatch(NONE_DECIDED)
    assert len(s.watches()) == 2 and len(c.watches()) == 3  # the clone has its own list
    assert c._signature(st) != s._signature(st)
    assert s.clearWatches() is s and s.watches() == [] and s._signature(st) == sig0
    # dsl_settings itself carries no watch: byte-identical with and without them
    assert bytes(c._encode(st)) == bytes(enc0)


def test_watch_encoding_is_the_predicates_own():
    p = PingPongIR(1, 10)
    st = p.initial_state()
    ws = watch_cases.pingpong_watches(p)
    s = SearchSettings()
    for w in ws:
        s.addWatch(w)
    key, arr, n, pool, n_pool = s._encode_watches(st)
    assert n == 8 and len(arr) == _lib.DSL_MAX_WATCHES and len(pool) == _lib.DSL_MAX_POOL
    assert s._encode_watches(st)[1] is arr  # cached while nothing changed
    ref_pool = []
    for i, w in enumerate(ws):
        e = w._encode(st, ref_pool)
        assert (arr[i].pred_id, arr[i].negate, arr[i].arg0, arr[i].arg1) == (e.pred_id, e.negate, e.arg0, e.arg1)
    assert n_pool == len(ref_pool) and [bytes(pool[i]) for i in range(n_pool)] == [bytes(q) for q in ref_pool]
    assert [arr[i].pred_id for i in range(8)] == [S.PRED_CLIENTS_DONE, S.PRED_FIELD, S.PRED_FIELD, S.PRED_FIELD, S.PRED_NET,
                                                  S.PRED_AND, S.PRED_FIELD, S.PRED_NET]
    assert arr[2].negate == 1 and arr[5].arg0 != arr[5].arg1
    # network leaves: consecutive record conditions of the WATCHES' pool
    for i in (4, 7):
        assert all(pool[arr[i].arg0 + k].pred_id == S.PRED_REC_COND for k in range(arr[i].arg1))
    other = SearchSettings().addWatch(ws[1])
    assert other._encode_watches(st)[0] != key  # the key is equal exactly when the encoded watches are
    assert SearchSettings().addWatch(ws[1])._encode_watches(st)[0] == other._encode_watches(st)[0]


def test_more_than_eight_watches_is_a_value_error():
    s = SearchSettings()
    for _ in range(8):
        s.addWatch(CLIENTS_DONE)
    with pytest.raises(ValueError, match="at most 8"):
        s.addWatch(CLIENTS_DONE)
    assert len(s.watches()) == 8
    mp = MultiPaxosIR(3, 2, "append-xy")
    two = mp.message("P2a").where(mp.message("P2a").field("round") >= 1)  # 2 conditions
    wide = S.allOf([two] * 13)  # 26 conditions + 24 operands: past the pool
    with pytest.raises(ValueError, match="pool entries"):
        SearchSettings().addWatch(wide)._encode_watches(mp.initial_state())


def test_results_without_watches_report_none():
    r = S.SearchResults(S.EndCondition.SPACE_EXHAUSTED, 3, [1, 2], 4, 5, None, None, 0.1, 2)
    assert r.watchCounts() == []
    r._watch_counts, r._watch_totals = [[0, 0], [0, 2], [1, 0]], [0, 3, 1]
    assert r.watchCounts() == [[0, 0], [0, 2], [1, 0]] and r.watchTotal(1) == 3
    assert [r.watchFirstDepth(i) for i in range(3)] == [None, 5, 4]  # absolute depths (initial_depth 4)


# ---- 2. the C ABI: two entry points, still ABI 6, no struct changed ---------------------------------------
def test_header_declares_the_entry_points_and_abi_stays_6():
    hdr = _header()
    assert int(re.search(r"#define DSL_ABI_VERSION (\d+)", hdr).group(1)) == 6 == _lib.DSL_ABI_VERSION
    assert int(re.search(r"#define DSL_MAX_WATCHES (\d+)", hdr).group(1)) == 8 == _lib.DSL_MAX_WATCHES
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int dsl_set_watches(dsl_engine* e, const dsl_predicate* watches, int32_t n_watches, "
            "const dsl_predicate* pool, int32_t n_pool);") in flat
    assert ("int dsl_watch_counts(dsl_engine* e, int32_t watch, uint64_t* per_depth, int32_t cap, "
            "int32_t* n_levels, uint64_t* total);") in flat
    assert "StatePredicate.java" in hdr and "Search.java:468-504" in hdr
    assert {"dsl_set_watches", "dsl_watch_counts"} <= set(_lib.EXPORTED)


def test_ctypes_prototypes_match_the_header(lib):
    P = ctypes.POINTER
    assert lib.dsl_set_watches.argtypes == [ctypes.c_void_p, P(_lib.dsl_predicate), ctypes.c_int32, P(_lib.dsl_predicate),
                                            ctypes.c_int32]
    assert lib.dsl_watch_counts.argtypes == [ctypes.c_void_p, ctypes.c_int32, P(ctypes.c_uint64), ctypes.c_int32,
                                             P(ctypes.c_int32), P(ctypes.c_uint64)]
    # a null engine is refused before anything is read
    assert lib.dsl_set_watches(None, None, 0, None, 0) == -1
    assert lib.dsl_watch_counts(None, 0, None, 0, None, None) == -1


def test_settings_and_result_structs_are_unchanged(tmp_path):
    """dsl_settings and dsl_result as the header had them before watches: the sizes and the last
    fields' offsets (include/dslabs_hip.h compiled with gcc) against the ctypes mirrors."""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dslabs_hip.h"', "int main(void) {",
           'printf("%zu %zu %zu %zu\\n", sizeof(dsl_settings), offsetof(dsl_settings, reserved), sizeof(dsl_result), '
           "offsetof(dsl_result, terminals)); return 0; }"]
    c = tmp_path / "abi.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.dsl_settings), _lib.dsl_settings.reserved.offset, ctypes.sizeof(_lib.dsl_result),
                   _lib.dsl_result.terminals.offset]
    assert not any("watch" in name for name, _ in _lib.dsl_settings._fields_ + _lib.dsl_result._fields_)


# ---- 3. the host's refusals and the kept `flat` (resolve_settings) ----------------------------------------
@pytest.fixture(scope="module", params=["plain", "ubsan"])
def watchcheck(request):
    return watch_cases.watchcheck_build(request.param)


def test_host_refuses_bad_watches_and_keeps_flat(watchcheck):
    p = subprocess.run([watchcheck, "refusals"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "runtime error" not in p.stderr, p.stdout + p.stderr
    out = json.loads(p.stdout)
    by = {r["case"]: r for r in out["refusals"]}
    want = {"nine watches": "outside 0..8", "bad field descriptor": "straddles a 32-bit word",
            "field beyond the node": "beyond the node", "unknown node": "node index",
            "record condition as a watch": "used as a predicate or a combinator operand",
            "combinator operand outside the pool": "combinator operand outside",
            "past 64 ops": "predicate programs too long", "past 32 network conditions": "more than 32 conditions in all"}
    assert set(want) <= set(by)
    for name, why in want.items():
        assert by[name]["rc"] == -1 and why in by[name]["why"], by[name]  # DSL_ERR_ARG, the fault named
        assert by[name]["untouched"] and by[name]["ok"], by[name]         # the resolved settings as they were
    assert by["32 conditions fit"]["ok"]
    # single-leaf invariants and prunes with a watch that is a tree: the flat judge stays on
    assert out["flat"] == 1 and out["n_ops"] == 8 and out["watch0_len"] == 5 and out["bad"] == 0


# ---- 4. the host census --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def census(watchcheck):
    rows = {}
    for name in watch_cases.CASES:
        proto, settings, state = watch_cases.case(name)
        rows[name] = watch_cases.watchcheck_run(watchcheck, name, proto, settings, state)
    return rows


@pytest.mark.parametrize("name", sorted(watch_cases.CASES))
def test_host_census_agrees_with_itself_and_the_fixture(census, name):
    row, gold = census[name], watch_cases.gold(name)
    assert row["mismatch"] == 0 and row["errors"] == 0 and row["evaluated"] > 0
    assert row["search_changed"] == 0  # the same per_depth and end with and without the watches
    assert row["per_depth"] == gold["per_depth"] and row["census"] == gold["census"] and row["true"] == gold["true"]
    _, settings, _ = watch_cases.case(name)
    assert gold["watches"] == [w.name for w in settings.watches()]
    assert all(len(c) == len(row["per_depth"]) for c in row["census"])
    assert all(t > 0 for t in row["true"])  # every watch of every case is reachable: each was true somewhere
    assert all(0 <= c <= n for vec in row["census"] for c, n in zip(vec, row["per_depth"]))


@pytest.mark.parametrize("cls", [MultiPaxos, MultiPaxosIR], ids=lambda c: c.__name__)
def test_host_census_of_the_mutant_is_the_oracles(watchcheck, cls):
    """mp_mut1_watch_logs: the log predicates FALSE, counted per depth by the oracle (which evaluates
    them in full) and by the host-compiled device predicates, on both forms of the protocol."""
    gold = watch_cases.gold("mp_mut1_watch_logs")
    proto, settings, state = watch_cases.mut1_watch_logs(cls)
    row = watch_cases.watchcheck_run(watchcheck, "mp_mut1_watch_logs", proto, settings, state)
    assert row["mismatch"] == 0 and row["errors"] == 0 and row["search_changed"] == 0
    assert row["per_depth"] == gold["per_depth"] and row["census"] == gold["census"]
    assert gold["watches"] == watch_cases.MUT_WATCHES
    # the first violation (depth 8: chosen without a majority) and, deeper, conflicting chosen commands
    assert gold["census"][0][:8] == [0] * 8 and gold["census"][0][8] > 0
    assert sum(gold["chosen_conflict"]) > 0
    assert all(a >= b for a, b in zip(gold["census"][0], gold["census"][1]))  # an invalid slot 1 is an inconsistent log


def test_fixture_per_depth_is_the_oracle_fixtures():
    assert watch_cases.gold("pp_1c10p_8w")["per_depth"] == watch_cases.fixture("lab0", "lab0_1c10p_exhaustive")["per_depth"]
    assert watch_cases.gold("pp_1c10p_goal")["per_depth"] == watch_cases.fixture("lab0", "lab0_1c10p_goal")["per_depth"]
    for name in ("mp_c5_d8_named", "mpir_c5_d8_named", "mpir_c5_d8_generic"):
        assert watch_cases.gold(name)["per_depth"] == watch_cases.fixture("multipaxos", "mp_c5_d8")["per_depth"]


def test_fixture_properties():
    pp = watch_cases.gold("pp_1c10p_8w")
    per, c = pp["per_depth"], pp["census"]
    assert c[3] == per                                            # results >= 0: every state
    assert [a + b for a, b in zip(c[1], c[2])] == per             # a watch plus its negation
    assert c[6][0] == 1                                           # results == 0 holds on the start state
    assert all(x <= y for x, y in zip(c[5], c[4]))                # a and !b is at most a
    named, ir, gen = (watch_cases.gold(n)["census"] for n in ("mp_c5_d8_named", "mpir_c5_d8_named", "mpir_c5_d8_generic"))
    assert named == ir                                            # hand-written and generated Multi-Paxos
    for k, (_, restates) in enumerate(watch_cases.MP_GENERIC):    # a generic restatement equals the named watch
        if restates:
            assert gen[k] == named[watch_cases.MP_NAMED.index(restates)], restates
    assert named[6] == [0] * 8 + [8]                              # CLIENTS_DONE: 8 of the 10,822 states of depth 8
    pb = watch_cases.gold("pb_2s1c_d6")["census"]
    assert pb[0] == pb[1]                                         # hasViewReply:1 and its raw-message restatement


# ---- 5. the oracle's goal searches anchor the named watches --------------------------------------------------
@pytest.mark.parametrize("key", sorted(watch_cases.ANCHORS))
def test_first_hit_matches_the_oracle_goal_search(key):
    """`bfs --goal P --finish-level` explores the same levels up to P's first hit: its depth and the
    number of distinct states holding P there are the census's first non-zero entry."""
    name, w = key
    depth, count = watch_cases.ANCHORS[key]
    want = oracle_util.run("bfs", watch_cases.ORACLE_ARGS[key], timeout=300)
    assert want["end"] == "GOAL_FOUND" and (want["max_depth"], want["num_terminals"]) == (depth, count)
    vec = watch_cases.gold(name)["census"][w]
    assert vec[:depth] == [0] * depth and vec[depth] == count
    assert want["per_depth"] == watch_cases.gold(name)["per_depth"][:depth + 1]
