"""Witnesses of the watches (SearchSettings.addWatch(p, witness=True) -> dsl_set_watch_witnesses /
dsl_watch_witness), the parts that need no GPU: the host truth of every case
(tests/hostcheck/witnesscheck.cpp: the minimum-fingerprint holder of each watch's first depth, chosen
two independent ways, also built with -fsanitize=undefined) against the committed
tests/golden/witness.json and the oracle's anchors, the mask encoding, the two entry points'
prototypes against the C header, and results without witnesses."""
import ctypes
import os
import re

import pytest

import watch_cases
import witness_cases
from dslabs_amd import CLIENTS_DONE, NONE_DECIDED, RESULTS_OK, SearchSettings, _lib
from dslabs_amd import search as S
from dslabs_amd.protocols import PingPongIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the host truth ------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "ubsan"])
def rows(request):
    exe = witness_cases.witnesscheck_build(request.param)
    return {name: witness_cases.witnesscheck_run(exe, name) for name in witness_cases.CASES}


@pytest.mark.parametrize("name", sorted(witness_cases.CASES))
def test_fixture_is_current_and_both_evaluations_agree(rows, name):
    row, gold = rows[name], witness_cases.gold(name)
    assert row["disagree"] == 0 and row["errors"] == 0
    assert row["per_depth"] == gold["per_depth"] and row["witnesses"] == gold["witnesses"]
    _, settings, _ = witness_cases.case(name)
    assert gold["watches"] == [w.name for w in settings.watches()] and len(gold["witnesses"]) == len(settings.watches())


@pytest.mark.parametrize("name", sorted(watch_cases.CASES))
def test_fixture_agrees_with_the_census_fixture(name):
    """The first depth and the holder count are the census's first non-zero entry (watch.json)."""
    wit, census = witness_cases.gold(name), watch_cases.gold(name)
    assert wit["per_depth"] == census["per_depth"]
    for w, vec in zip(wit["witnesses"], census["census"]):
        first = next((i for i, c in enumerate(vec) if c), None)
        assert first is not None and (w["first_depth"], w["holders"]) == (first, vec[first])
        assert w["trace_len"] == first and len(bytes.fromhex(w["state"])) > 0


def test_fixture_first_depths_and_holders_are_the_oracles_anchors():
    many = 0
    for (name, w), (depth, count) in watch_cases.ANCHORS.items():
        row = witness_cases.gold(name)["witnesses"][w]
        assert (row["first_depth"], row["holders"]) == (depth, count), (name, w)
        many += 2 <= count <= 8
    # the choice among candidates is exercised: the seven Multi-Paxos anchors and PB's have 2 to 8 holders
    assert len(watch_cases.ANCHORS) == 9 and many == 8


def test_fixture_properties():
    extra = witness_cases.gold("pp_1c10p_extra")["witnesses"]
    assert extra[0] == {"first_depth": -1, "holders": 0}                  # no reachable state holds it
    assert extra[1]["first_depth"] == 0 and extra[1]["trace_len"] == 0  # the start state
    p = PingPongIR(1, 10)
    assert bytes.fromhex(extra[1]["state"]) == p.initial_state()._packed_now()
    assert extra[2] == witness_cases.gold("pp_1c10p_8w")["witnesses"][0] == witness_cases.gold("pp_1c10p_goal")["witnesses"][0]
    named, gen = witness_cases.gold("mpir_c5_d8_named")["witnesses"], witness_cases.gold("mpir_c5_d8_generic")["witnesses"]
    for k, (_, restates) in enumerate(watch_cases.MP_GENERIC):  # a generic restatement picks the named watch's state
        if restates:
            assert gen[k] == named[watch_cases.MP_NAMED.index(restates)], restates
    # hand-written and generated Multi-Paxos pack differently, but agree on depths and counts
    hand = witness_cases.gold("mp_c5_d8_named")["witnesses"]
    assert [(w["first_depth"], w["holders"]) for w in hand] == [(w["first_depth"], w["holders"]) for w in named]
    pb = witness_cases.gold("pb_2s1c_d6")["witnesses"]
    assert pb[0] == pb[1] and pb[0]["first_depth"] == 1 and pb[0]["holders"] == 2


# ---- 2. the Python encoding ----------------------------------------------------------------------------------
def test_mask_clone_and_signature():
    p = PingPongIR(1, 10)
    st = p.initial_state()
    done = p.length("client1", "_results") == 10
    s = SearchSettings().addInvariant(RESULTS_OK)
    assert s._witness_mask() == 0
    assert s.addWatch(CLIENTS_DONE, witness=True).addWatch(done).addWatch(NONE_DECIDED, witness=True) is s
    assert s._witness_mask() == 0b101 and s.watches() == [CLIENTS_DONE, done, NONE_DECIDED]
    c = s.clone()
    assert c._witness_mask() == 0b101 and c._signature(st) == s._signature(st)
    c.addWatch(done, witness=True)
    assert c._witness_mask() == 0b1101 and s._witness_mask() == 0b101  # the clone has its own flags
    plain = SearchSettings().addInvariant(RESULTS_OK).addWatch(CLIENTS_DONE).addWatch(done).addWatch(NONE_DECIDED)
    assert plain._signature(st) != s._signature(st)  # the requests are part of what a search is
    assert plain._encode_watches(st)[0] == s._encode_watches(st)[0]  # ... and no part of the watches' encoding
    assert len(s._encode_watches(st)) == 5
    assert s.clearWatches()._witness_mask() == 0 and s.watches() == []
    every = witness_cases.with_witnesses(plain)
    assert every._witness_mask() == 0b111 and plain._witness_mask() == 0
    assert witness_cases.with_witnesses(plain, which={1})._witness_mask() == 0b010


def test_add_watch_without_the_keyword_is_as_before():
    s = SearchSettings().addWatch(CLIENTS_DONE)
    assert s.watches() == [CLIENTS_DONE] and s._witness_mask() == 0 and s._witness == [False]
    with pytest.raises(ValueError, match="at most 8"):
        for _ in range(8):
            s.addWatch(CLIENTS_DONE, witness=True)
    assert len(s.watches()) == 8 == len(s._witness) and s._witness_mask() == 0xfe


def test_results_without_witnesses():
    r = S.SearchResults(S.EndCondition.SPACE_EXHAUSTED, 3, [1, 2], 4, 5, None, None, 0.1, 2)
    assert r.watchWitness(0) is None and r.watchWitness(7) is None
    for bad in (-1, 8):
        with pytest.raises(ValueError, match="watchWitness"):
            r.watchWitness(bad)
    r._watch_counts, r._watch_totals = [[0, 0], [0, 2]], [0, 2]  # two watches, no witness requested
    assert r.watchWitness(0) is None and r.watchWitness(1) is None
    with pytest.raises(ValueError, match="watch 2 of 2"):
        r.watchWitness(2)
    w = S.SearchState(PingPongIR(1, 10), b"\0" * 8, 5)
    r._witnesses = [None, w]
    assert r.watchWitness(0) is None and r.watchWitness(1) is w


# ---- 3. the C ABI: two more entry points, still ABI 6 -----------------------------------------------------------
def test_header_declares_the_entry_points_and_abi_stays_6():
    with open(os.path.join(ROOT, "include", "dslabs_hip.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define DSL_ABI_VERSION (\d+)", hdr).group(1)) == 6 == _lib.DSL_ABI_VERSION
    flat = re.sub(r"\s+", " ", hdr)
    assert "int dsl_set_watch_witnesses(dsl_engine* e, uint32_t mask);" in flat
    assert ("int dsl_watch_witness(dsl_engine* e, int32_t watch, int32_t* depth, dsl_event* trace, int32_t cap, "
            "int32_t* trace_len, uint8_t* state, size_t len);") in flat
    assert "Still 6 with dsl_set_watch_witnesses / dsl_watch_witness" in flat
    assert {"dsl_set_watch_witnesses", "dsl_watch_witness"} <= set(_lib.EXPORTED)


def test_library_exports_both_and_refuses_a_null_engine(lib):
    P = ctypes.POINTER
    assert lib.dsl_set_watch_witnesses.argtypes == [ctypes.c_void_p, ctypes.c_uint32]
    assert lib.dsl_watch_witness.argtypes == [ctypes.c_void_p, ctypes.c_int32, P(ctypes.c_int32), P(_lib.dsl_event),
                                              ctypes.c_int32, P(ctypes.c_int32), P(ctypes.c_uint8), ctypes.c_size_t]
    assert lib.dsl_set_watch_witnesses(None, 1) == -1
    depth = ctypes.c_int32(7)
    assert lib.dsl_watch_witness(None, 0, ctypes.byref(depth), None, 0, None, None, 0) == -1
    assert depth.value == 7  # refused before anything is written
