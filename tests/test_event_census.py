"""The event census (SearchSettings.eventCensus -> dsl_set_event_census / dsl_event_census), the
parts that need no GPU: the host truth of every case (tests/hostcheck/eventcheck.cpp: a
breadth-first walk with exact state equality, also built with -fsanitize=undefined) tied to the
oracle's committed per_depth and compared with the committed tests/golden/event_census.json, the
census's identities on that fixture, the class names against the rendered events of every
committed trace, the Python encoding, and the five entry points against the C header."""
import ctypes
import glob
import json
import os
import re

import pytest

import argmap
import event_cases
from dslabs_amd import RESULTS_OK, EventCount, SearchSettings, _lib
from dslabs_amd import search as S
from dslabs_amd.protocols import (PB, PBIR, AmoKV, AmoKVIR, MiniTest, MultiPaxos, MultiPaxosIR, PingPong, PingPongIR,
                                  SIPaxos, Synthetic)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(event_cases.CASES)
PROTOCOLS = [PingPong(1, 10), SIPaxos(), MultiPaxos(3, 2, "append-xy"), Synthetic(), AmoKV(), PB(2, 1, "putget"), MiniTest(),
             PingPongIR(1, 10), AmoKVIR(), MultiPaxosIR(3, 2, "append-xy"), PBIR(2, 1, "putget")]


# ---- 1. the host truth ------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "ubsan"])
def rows(request, lib):
    exe = event_cases.eventcheck_build(request.param)
    out = {}
    for name in event_cases.CASES:  # in order: pb_stage2 starts from this walk's pb_initview terminal
        goal = out["pb_initview"]["terminal"] if name == "pb_stage2" else None
        out[name] = event_cases.eventcheck_run(exe, name, goal)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_walk_reproduces_the_oracles_per_depth(rows, name):
    want = event_cases.fixture_per_depth(name)
    if want is not None:
        assert rows[name]["per_depth"] == want
    else:  # no oracle fixture of its own: the committed census fixture pins it
        assert rows[name]["per_depth"] == event_cases.gold(name)["per_depth"]


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_current(rows, name):
    row, gold = rows[name], event_cases.gold(name)
    assert row["errors"] == 0
    for k in gold:
        assert row[k] == gold[k], k


def test_every_device_protocol_has_a_case():
    seen = {argmap.protocol(args).proto_id for args, _ in event_cases.CASES.values()}
    assert seen == {p.proto_id for p in PROTOCOLS} and len(seen) == 11


@pytest.mark.parametrize("name", NAMES)
def test_identities_hold_in_the_fixture(name):
    g = event_cases.gold(name)
    dense = [event_cases.dense(r, g["classes"], g["nodes"]) for r in g["rows"]]
    event_cases.check_identities(dense, g["per_depth"], g["successors"])
    # one row per expanded level: every depth but the last was expanded, and the last one too unless
    # the search stopped there (maxDepth, a terminal level, or an empty frontier after it)
    assert len(g["per_depth"]) - 1 <= len(g["rows"]) <= len(g["per_depth"])
    proto, _, _ = event_cases.case(name)
    assert g["classes"] == len(proto.event_classes()) and g["nodes"] == len(proto.addresses)


def test_fixture_properties():
    g = event_cases.gold()
    # the generated protocols count what the hand-written ones count, class by class where the
    # classes line up (PingPong, AmoKV and PB: the same message types and one timer class)
    for a, b in (("lab0_1c10p_exhaustive", "lab0_1c10p_exhaustive_ir"), ("lab0_2c10p_exhaustive", "lab0_2c10p_exhaustive_ir"),
                 ("kv_test09", "kv_test09_ir"), ("pb_2s1c_d7", "pb_2s1c_d7_ir")):
        assert g[a]["rows"] == g[b]["rows"] and g[a]["successors"] == g[b]["successors"]
    # Multi-Paxos: the generated form has one timer class where the hand-written one has two
    hand, gen = g["mp_c5_d8"], g["mp_c5_d8_ir"]
    fold = [sorted([c if c < 9 else 8, t] + v for c, t, *v in row) for row in hand["rows"]]
    assert fold == [sorted(row) for row in gen["rows"]] and hand["classes"] == 10 and gen["classes"] == 9
    # MiniTest: a's Foo handler throws; the level completes and the search ends on the exception
    mini = g["minitest"]
    assert mini["end"] == 2 and mini["rows"][1][0] == [0, 0, 1, 0, 1, 0] and len(mini["rows"]) == 2
    assert sum(c[4] for n in g for row in g[n]["rows"] for c in row) == 1  # the only exceptional step of all cases
    # the closed links' and the silenced timers' cells are zero in every row, and not in the open search
    for name, cells in event_cases.ZERO_CELLS.items():
        proto, _, _ = event_cases.case(name)
        cls = [n for n, _ in proto.event_classes()]
        for cname, addr in cells:
            key = [cls.index(cname), proto.addresses.index(addr)]
            assert all(c[:2] != key for row in g[name]["rows"] for c in row), (name, cname, addr)
    mp = MultiPaxos(3, 2, "append-xy")
    cls = [n for n, _ in mp.event_classes()]
    for cname, addr in event_cases.ZERO_CELLS["mp_c5_d6_cut"]:
        key = [cls.index(cname), mp.addresses.index(addr)]
        assert any(c[:2] == key for row in hand["rows"][:6] for c in row), (cname, addr)
    # the second stage starts at initView's terminal depth and its first row is that depth's
    assert g["pb_stage2"]["initial_depth"] == g["pb_initview"]["terminal"]["depth"] == 11 and len(g["pb_stage2"]["rows"]) == 5
    assert g["pb_initview"]["end"] == 4 and len(g["pb_initview"]["rows"]) == 11  # the goal's level is a completed level
    # C5's frontiers: chunks that do not divide them, several segments, many workgroups
    assert {5, 66, 207, 4050} <= set(hand["per_depth"][:8]) and sum(hand["per_depth"]) == 17320


# ---- 2. class names ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("proto", PROTOCOLS, ids=lambda p: type(p).__name__)
def test_class_names_and_timer_split(lib, proto):
    d = proto.desc()
    n = lib.dsl_event_class_count(ctypes.byref(d))
    classes = proto.event_classes()
    assert 2 <= n <= _lib.DSL_EVENT_CLASSES and len(classes) == n and len(proto.addresses) <= _lib.DSL_EVENT_NODES
    assert all(name and re.fullmatch(r"[A-Za-z0-9|]+", name) for name, _ in classes)
    assert len({name for name, _ in classes}) == n
    for bad in (-1, n, n + 1, 1 << 20):
        assert lib.dsl_event_class_name(ctypes.byref(d), bad) is None
        assert lib.dsl_event_class_is_timer(ctypes.byref(d), bad) == -1
    # messages first, then the timer classes: is_timer splits at kMsgClasses
    flags = [t for _, t in classes]
    k = flags.index(True)
    assert flags == [False] * k + [True] * (n - k) and 1 <= k < n
    src = {"PingPong": "pingpong.hpp", "SIPaxos": "sipaxos.hpp", "MultiPaxos": "multipaxos.hpp", "Synthetic": "synthetic.hpp",
           "AmoKV": "amokv.hpp", "PB": "pb.hpp", "MiniTest": "minitest.hpp", "PingPongIR": "gen/pingpong_ir.hpp",
           "AmoKVIR": "gen/amokv_ir.hpp", "MultiPaxosIR": "gen/multipaxos_ir.hpp", "PBIR": "gen/pb_ir.hpp"}[type(proto).__name__]
    with open(os.path.join(ROOT, "dslabs_amd", "csrc", "protocols", src)) as f:
        assert k == int(re.search(r"kMsgClasses = (\d+)", f.read()).group(1))


def test_unknown_protocol_has_no_classes(lib):
    d = _lib.dsl_protocol_desc()
    d.protocol = 99
    assert lib.dsl_event_class_count(ctypes.byref(d)) == -6 and lib.dsl_event_class_name(ctypes.byref(d), 0) is None
    assert lib.dsl_event_class_count(None) == -1 and lib.dsl_event_class_name(None, 0) is None
    assert lib.dsl_event_class_is_timer(None, 0) == -1


def test_every_committed_trace_renders_with_its_class_name():
    """Every event of every trace in the oracle fixtures is called what exactly one class of its
    kind (message / timer) is called, and a message's class is its type's."""
    pat = re.compile(r"^(Message|Timer)\((?:[\w-]+ )?-> [\w-]+, (\w+)\(")
    checked = 0
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.json"))):
        with open(path) as f:
            data = json.load(f)
        for row in (data.values() if isinstance(data, dict) else []):
            if not (isinstance(row, dict) and row.get("args") and "terminals" in row):
                continue
            classes = argmap.protocol(row["args"]).event_classes()
            for term in row["terminals"]:
                for line in term.get("trace", []):
                    m = pat.match(line)
                    assert m, line
                    hits = [c for c, (name, is_timer) in enumerate(classes)
                            if is_timer == (m.group(1) == "Timer") and m.group(2) in name.split("|")]
                    assert len(hits) == 1, (line, classes)
                    checked += 1
    assert checked >= 400  # the fixtures hold 414 trace events


def test_rendered_events_of_a_generated_protocol_use_its_class_names():
    mp = MultiPaxosIR(3, 2, "append-xy")
    classes = mp.event_classes()
    for t, m in enumerate(mp.spec.messages):
        e = _lib.dsl_event()
        e.type, e.from_, e.to = t, 0, 1
        assert classes[t] == (m.name, False) and f", {m.name}(" in mp.render_event(e)
    for k, tm in enumerate(mp.spec.timers):
        e = _lib.dsl_event()
        e.is_timer, e.type, e.to = 1, len(mp.spec.messages) + k, 0
        assert tm.name in classes[-1][0].split("|") and f", {tm.name}(" in mp.render_event(e)


# ---- 3. the Python encoding ----------------------------------------------------------------------------------
def test_event_census_clone_and_signature():
    p = PingPongIR(1, 10)
    st = p.initial_state()
    s = SearchSettings().addInvariant(RESULTS_OK)
    sig0, enc0 = s._signature(st), bytes(s._encode(st))
    assert s._event_census is False and s.eventCensus() is s and s._event_census is True
    assert s._signature(st) != sig0  # the census is part of what a search is
    c = s.clone()
    assert c._event_census and c._signature(st) == s._signature(st)
    assert c.eventCensus(False)._event_census is False and s._event_census and c._signature(st) == sig0
    assert bytes(s._encode(st)) == enc0  # dsl_settings itself carries no census: byte-identical


def test_results_without_a_census_and_the_dict_forms():
    r = S.SearchResults(S.EndCondition.SPACE_EXHAUSTED, 3, [1, 2], 4, 5, None, None, 0.1, 2)
    assert r.eventRows() == [] and r.eventCensus() == [] and r.eventTotals() == {}
    r._event_classes, r._event_addresses = [("Ping", False), ("Tick", True)], ["a", "b"]
    r._event_rows = [[[(3, 1, 0, 2), (0, 0, 0, 0)], [(0, 0, 0, 0), (4, 0, 1, 1)]],
                     [[(5, 5, 0, 0), (0, 0, 0, 0)], [(0, 0, 0, 0), (0, 0, 0, 0)]]]
    assert r.eventCensus() == [{("Ping", "a"): EventCount(3, 1, 0, 2), ("Tick", "b"): EventCount(4, 0, 1, 1)},
                               {("Ping", "a"): EventCount(5, 5, 0, 0)}]
    assert r.eventTotals() == {("Ping", "a"): EventCount(8, 6, 0, 2), ("Tick", "b"): EventCount(4, 0, 1, 1)}
    assert EventCount(4, 0, 1, 1).revisits == 2 and EventCount(8, 6, 0, 2).revisits == 0
    rows = r.eventRows()
    rows[0][0][0] = 99  # a copy
    assert r.eventRows()[0][0][0] == (3, 1, 0, 2)


# ---- 4. the C ABI: five more entry points, still ABI 6 ---------------------------------------------------------
def test_header_declares_the_entry_points_and_abi_stays_6():
    with open(os.path.join(ROOT, "include", "dslabs_hip.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define DSL_ABI_VERSION (\d+)", hdr).group(1)) == 6 == _lib.DSL_ABI_VERSION
    assert int(re.search(r"#define DSL_EVENT_CLASSES (\d+)", hdr).group(1)) == 15 == _lib.DSL_EVENT_CLASSES
    assert int(re.search(r"#define DSL_EVENT_NODES (\d+)", hdr).group(1)) == 8 == _lib.DSL_EVENT_NODES
    flat = re.sub(r"\s+", " ", hdr)
    for decl in ("typedef struct { uint64_t events, noops, exceptions, fresh; } dsl_event_count;",
                 "int dsl_event_class_count(const dsl_protocol_desc* proto);",
                 "const char* dsl_event_class_name(const dsl_protocol_desc* proto, int32_t cls);",
                 "int dsl_event_class_is_timer(const dsl_protocol_desc* proto, int32_t cls);",
                 "int dsl_set_event_census(dsl_engine* e, int32_t on);",
                 "int dsl_event_census(dsl_engine* e, int32_t level, dsl_event_count* cells, int32_t* n_levels);"):
        assert decl in flat, decl
    assert "Still 6 with dsl_set_watch_witnesses / dsl_watch_witness" in flat
    assert "Still 6 with dsl_set_event_census / dsl_event_census" in flat
    new = {"dsl_event_class_count", "dsl_event_class_name", "dsl_event_class_is_timer", "dsl_set_event_census",
           "dsl_event_census"}
    assert new <= set(_lib.EXPORTED)
    import dslabs_amd
    assert "EventCount" in dslabs_amd.__all__
    # the structs keep their bytes
    assert ctypes.sizeof(_lib.dsl_event_count) == 32


def test_ctypes_prototypes_and_null_engine_refusals(lib):
    P = ctypes.POINTER
    assert lib.dsl_event_class_count.argtypes == [P(_lib.dsl_protocol_desc)]
    assert lib.dsl_event_class_name.argtypes == [P(_lib.dsl_protocol_desc), ctypes.c_int32]
    assert lib.dsl_event_class_name.restype == ctypes.c_char_p
    assert lib.dsl_event_class_is_timer.argtypes == [P(_lib.dsl_protocol_desc), ctypes.c_int32]
    assert lib.dsl_set_event_census.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert lib.dsl_event_census.argtypes == [ctypes.c_void_p, ctypes.c_int32, P(_lib.dsl_event_count), P(ctypes.c_int32)]
    assert lib.dsl_set_event_census(None, 1) == -1
    assert b"dsl_set_event_census" in lib.dsl_last_error()
    n = ctypes.c_int32(7)
    assert lib.dsl_event_census(None, 0, None, ctypes.byref(n)) == -1 and n.value == 0
    assert b"dsl_event_census" in lib.dsl_last_error()
