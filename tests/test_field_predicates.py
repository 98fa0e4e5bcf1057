"""User-written field predicates (FieldRef comparisons -> DSL_PRED_FIELD), the parts that need no
GPU: the layout resolution against the generated device headers, the descriptor encoding against
the C header's macros, the Python-side errors, the shared judge on the host (tools/cpu_bfs.cpp)
against the golden fixtures, and the stand-alone host check (tests/hostcheck/fieldcheck.cpp), also
built with -fsanitize=undefined."""
import json
import os
import re
import subprocess

import pytest

import field_cases
from dslabs_amd import (CLIENTS_DONE, FieldRef, SearchSettings, StatePredicate, allOf, anyOf, field_value,
                        statePredicate)
from dslabs_amd import search as S
from dslabs_amd.protocols import (PB, AmoKV, MiniTest, MultiPaxos, MultiPaxosIR, PingPong, PingPongIR, SIPaxos,
                                  Synthetic)
from tools import cpu_baseline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "dslabs_amd", "csrc", "protocols", "gen")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _gen(name):
    with open(os.path.join(GEN, name)) as f:
        return f.read()


# ---- 1. layout resolution ------------------------------------------------------------------------
def test_pingpong_results_length_is_what_the_generated_header_reads():
    r = PingPongIR(1, 10).length("client1", "_results")
    assert (r.node, r.bit, r.width) == (1, 96, 4)
    assert "get(w, 96, 4)" in _gen("pingpong_ir.hpp")
    assert repr(r) == "length(client1._results)"
    assert repr(r == 10) == "length(client1._results) == 10"


def test_multipaxos_fields_are_what_the_generated_header_reads():
    p = MultiPaxosIR(3, 2, "append-xy")
    src = _gen("multipaxos_ir.hpp")
    # a client's harvested results' length: the header's predicates read get(pn_client_0, 26, 2)
    r = p.length("client1", "_results")
    assert (r.node, r.bit, r.width) == (3, 26, 2)
    assert f"get(pn_client_0, {r.bit}, {r.width})" in src
    # a server scalar: slotin is the header's `int l_slot = get(w, 17, 3)` (the proposer's next slot)
    f = p.field("server2", "slotin")
    assert (f.node, f.bit, f.width) == (1, 17, 3)
    assert re.search(r"int l_slot = get\(w, 17, 3\);", src)
    # the log array: arr_server_log reads an 11-bit element at (j / 2 * 32 + j % 2 * 11) of the window at w[1]
    m = re.search(r"arr_server_log\(const uint32_t\* w, int j\) \{\s*return \(int\)\(\(\(\(uint64_t\)w\[(\d)\] \| "
                  r"\(\(uint64_t\)w\[\d\] << 32\)\) >> \((\d+) \+ \(j\) / (\d+) \* 32 \+ \(j\) % \d+ \* (\d+)\)\) & (\d+)u\);",
                  src)
    word, off, per, bits, mask = (int(x) for x in m.groups())
    for j in range(4):
        e = p.field("server1", "log", j)
        assert (e.node, e.bit, e.width) == (0, 32 * word + off + j // per * 32 + j % per * bits, bits)
        assert mask == (1 << e.width) - 1
    # sub-fields of a log entry (ir/specs/multipaxos.py st / eb / ec: status 0-1, ballot 2-7, command 8-10)
    e = p.field("server3", "log", 1)
    assert [(x.bit - e.bit, x.width) for x in (e.bits(0, 2), e.bits(2, 6), e.bits(8, 3))] == [(0, 2), (2, 6), (8, 3)]
    assert repr(e.bits(8, 3) == 1) == "server3.log[1][8:11] == 1"
    assert repr(p.field("server2", "round") <= 3) == "server2.round <= 3"


def test_node_words_match_the_device_protocols():
    """Protocol.node_words (field_value, raw_field's range check) is the device struct's kNodeWords."""
    csrc = os.path.join(ROOT, "dslabs_amd", "csrc", "protocols")
    for proto, path, struct in ((PingPong(), "pingpong.hpp", "PingPong"), (SIPaxos(), "sipaxos.hpp", "SIPaxos"),
                                (MultiPaxos(), "multipaxos.hpp", "MultiPaxos"), (Synthetic(), "synthetic.hpp", "Synthetic"),
                                (AmoKV(), "amokv.hpp", "AmoKV"), (PB(), "pb.hpp", "PB"), (MiniTest(), "minitest.hpp", "MiniTest"),
                                (PingPongIR(), "gen/pingpong_ir.hpp", "PingPongIR"),
                                (MultiPaxosIR(), "gen/multipaxos_ir.hpp", "MultiPaxosIR")):
        with open(os.path.join(csrc, path)) as f:
            body = f.read().split(f"struct {struct} {{", 1)[1]
        assert proto.node_words == int(re.search(r"kNodeWords = (\d+)", body).group(1)), struct


def test_descriptor_macros_round_trip(tmp_path):
    """The C header's DSL_FIELD_* macros and the Python encoding agree, both ways."""
    cases = [(0, 0, 1, S.CMP_EQ, 0), (31, 65535 - 31, 32, S.CMP_GT, 1), (4, 96, 4, S.CMP_LE, 0), (17, 171, 11, S.CMP_GE, 1),
             (1, 32, 32, S.CMP_NE, 0), (2, 63, 1, S.CMP_LT, 1)]
    src = ['#include <stdio.h>', '#include "dslabs_hip.h"', "int main(void) {"]
    for node, bit, width, cmp, rhs in cases:
        src.append(f"{{ uint32_t d = DSL_FIELD_DESC({node}, {bit}, {width}); int64_t a = DSL_FIELD_ARG0(d, {cmp}, {rhs});"
                   ' printf("%u %lld %d %d %d %u %d %d\\n", d, (long long)a, DSL_FIELD_NODE(d), DSL_FIELD_BIT(d),'
                   " DSL_FIELD_WIDTH(d), DSL_FIELD_ARG0_DESC(a), DSL_FIELD_ARG0_CMP(a), DSL_FIELD_ARG0_RHS_IS_FIELD(a)); }")
    src.append('printf("%d %d %d %d %d %d %d\\n", DSL_PRED_FIELD, DSL_CMP_EQ, DSL_CMP_NE, DSL_CMP_LT, DSL_CMP_GE, DSL_CMP_LE,'
               " DSL_CMP_GT); return 0; }")
    c = tmp_path / "desc.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    for (node, bit, width, cmp, rhs), line in zip(cases, lines):
        d, a, n2, b2, w2, d2, c2, r2 = (int(x) for x in line.split())
        assert d == S.field_desc(node, bit, width) and a == S.field_arg0(d, cmp, bool(rhs))
        assert (n2, b2, w2) == (node, bit, width) == S.field_desc_decode(d)
        assert (d2, c2, bool(r2)) == (d, cmp, bool(rhs)) == S.field_arg0_decode(a)
        assert d <= 0x07FFFFFF and 0 <= a < 1 << 36
    assert [int(x) for x in lines[-1].split()] == [S.PRED_FIELD, S.CMP_EQ, S.CMP_NE, S.CMP_LT, S.CMP_GE, S.CMP_LE,
                                                   S.CMP_GT]


def test_java_constants_match_the_header():
    with open(os.path.join(ROOT, "java", "src", "dslabs", "framework", "testing", "search", "gpu",
                           "GpuPredicates.java")) as f:
        java = f.read()
    with open(os.path.join(ROOT, "include", "dslabs_hip.h")) as f:
        hdr = f.read()
    pred_field = int(re.search(r"DSL_PRED_FIELD = (\d+)", hdr).group(1))
    assert pred_field == S.PRED_FIELD and "FIELD = %d;" % pred_field in java
    cmp = {n: int(re.search(r"#define DSL_CMP_%s (\d)" % n, hdr).group(1)) for n in ("EQ", "NE", "LT", "GE", "LE", "GT")}
    assert ", ".join(f"CMP_{n} = {v}" for n, v in cmp.items()) + ";" in java
    assert "((long) node << 22) | ((long) width << 16) | bit" in java  # DSL_FIELD_DESC
    assert "((long) cmp << 32) | (1L << 35)" in java                   # DSL_FIELD_ARG0


def test_comparisons_encode_as_documented():
    p = MultiPaxosIR()
    a, b = p.field("server1", "leader"), p.field("server2", "leader")
    for op, cmp in (("eq", S.CMP_EQ), ("ne", S.CMP_NE), ("lt", S.CMP_LT), ("le", S.CMP_LE), ("gt", S.CMP_GT),
                    ("ge", S.CMP_GE)):
        k = getattr(a, op)(2)
        assert k.pred_id == S.PRED_FIELD and S.field_arg0_decode(k.arg0) == (a.desc(), cmp, False) and k.arg1 == 2
        ff = getattr(a, op)(b)
        assert S.field_arg0_decode(ff.arg0) == (a.desc(), cmp, True) and ff.arg1 == b.desc()
    assert (a == 2).arg0 == a.eq(2).arg0 and (a != b).arg0 == a.ne(b).arg0 and (a < 1).arg0 == a.lt(1).arg0
    assert (a <= b).arg0 == a.le(b).arg0 and (a > 0).arg0 == a.gt(0).arg0 and (a >= b).arg0 == a.ge(b).arg0
    assert (a == 0xFFFFFFFF).arg1 == 0xFFFFFFFF
    # the C ABI form: a leaf, negated, renamed, inside combinators
    st = p.initial_state()
    pool = []
    enc = (a <= 3).negate()._encode(st, pool)
    assert (enc.pred_id, enc.negate, enc.arg0, enc.arg1, pool) == (950, 1, (a <= 3).arg0, 3, [])
    named = statePredicate("leaders agree", a == b)
    assert named.name == "leaders agree" and (named.pred_id, named.arg0, named.arg1) == (950, (a == b).arg0, b.desc())
    assert named.negate().name == "¬(leaders agree)" and named.negate().negated
    both = allOf([a == 1, b == 1, a >= b])
    assert both.pred_id == S.PRED_AND and both.operands[0].pred_id == S.PRED_AND and both.operands[1].pred_id == 950
    either = anyOf([a == 1, b == 1])
    assert either.pred_id == S.PRED_OR and [o.pred_id for o in either.operands] == [950, 950]
    assert allOf([a == 1]).pred_id == 950
    assert isinstance(a, FieldRef) and isinstance(a == b, StatePredicate)


def test_errors_are_raised_in_python():
    pp, mp = PingPongIR(2, 10), MultiPaxosIR(3, 2)
    bad = [
        lambda: pp.field("client3", "ping"),                    # unknown address (2 clients)
        lambda: pp.length("nobody", "_results"),
        lambda: Synthetic(3).raw_field("node4", 0, 16),
        lambda: Synthetic(3).raw_field(3, 0, 16),
        lambda: pp.field("pingserver", "ping"),                 # a field the kind does not have
        lambda: mp.field("client1", "round"),
        lambda: mp.length("server1", "_timers"),                # the server keeps no timer queue (fixed Tick)
        lambda: mp.length("server1", "log"),                    # an array has no length
        lambda: mp.length("server1", "round"),
        lambda: mp.field("server1", "log", 4),                  # index out of range
        lambda: mp.field("server1", "log", -1),
        lambda: mp.field("server1", "log"),                     # a list needs an index
        lambda: mp.field("server1", "round", 0),                # a scalar takes none
        lambda: pp.field("client1", "_results", 15),
        lambda: pp.field("client1", "ping") == 1 << 32,         # constants: 32 unsigned bits
        lambda: pp.field("client1", "ping") < -1,
        lambda: mp.field("server1", "log", 0).bits(8, 4),       # bits() outside the field
        lambda: mp.field("server1", "log", 0).bits(-1, 2),
        lambda: mp.field("server1", "log", 0).bits(0, 0),
        lambda: Synthetic(3).raw_field("node1", 0, 33),         # raw fields: width, straddle, node size
        lambda: Synthetic(3).raw_field("node1", 0, 0),
        lambda: Synthetic(3).raw_field("node1", 30, 4),
        lambda: Synthetic(3).raw_field("node1", 64, 8),
        lambda: Synthetic(3).raw_field("node1", -1, 8),
        lambda: pp.field("client1", "ping") == mp.field("server1", "round"),  # two protocols
        lambda: allOf([]),
        lambda: anyOf([]),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {k} raised nothing")
    with pytest.raises(TypeError):
        pp.field("client1", "ping") == "1"
    # the limits of the C ABI keep their messages
    ping = pp.field("client1", "ping")
    with pytest.raises(ValueError, match="too many predicates"):
        s = SearchSettings()
        for j in range(17):
            s.addInvariant(ping != j)
        s._encode(pp.initial_state())
    with pytest.raises(ValueError, match="too many combinator operands"):
        SearchSettings().addInvariant(anyOf([ping == j % 16 for j in range(26)]))._encode(pp.initial_state())


def test_field_value_decodes_the_packed_state():
    """field_value on the initial states (dsl_init_state: host only), against the specs' init handlers."""
    pp = PingPongIR(1, 10)
    st = pp.initial_state()
    # ClientWorker sent command 1: ping = 1, pong = 0, one PingTimer, no results
    assert [field_value(st, pp.field("client1", n)) for n in ("ping", "pong")] == [1, 0]
    assert field_value(st, pp.length("client1", "_timers")) == 1 and field_value(st, pp.length("client1", "_results")) == 0
    assert field_value(st, pp.raw_field("client1", 0, 32)) == 1 | (1 << 8)  # word 0: ping = 1, one timer
    assert field_value(st, pp.field("client1", "_timers", 0)) == 1          # PingTimer(1)
    sy = Synthetic(3)
    assert field_value(sy.initial_state(), sy.raw_field("node2", 32, 8)) == 0 | (1 << 2) | (2 << 4) | (3 << 6)  # synthetic.hpp init


# ---- 2. the shared judge on the host: golden fixtures restated ------------------------------------
@pytest.mark.parametrize("name", sorted(field_cases.CASES))
def test_cpu_judge_matches_golden_with_field_predicates(name):
    gold, proto, settings = field_cases.case(name)
    r = cpu_baseline.run(proto, settings, threads=2, table_log2=20)
    assert r["end"] == gold["end"]
    assert r["per_depth"] == gold["per_depth"]
    assert r["states"] == gold["states"]
    if gold["terminal_depth"] >= 0:  # cpu_bfs finishes the terminal's level and stops
        assert len(r["per_depth"]) - 1 == gold["terminal_depth"]


def test_pinned_counts_of_the_issue():
    """The fixtures the restated cases run against say what the issue quotes."""
    g = field_cases.gold
    assert (g("lab0", "lab0_1c10p_goal")["states"], g("lab0", "lab0_1c10p_goal")["terminal_depth"]) == (84, 20)
    assert (g("lab0", "lab0_1c10p_exhaustive")["states"], g("lab0", "lab0_1c10p_exhaustive")["max_depth"]) == (120, 29)
    assert g("lab0", "lab0_2c10p_exhaustive")["states"] == 14640


def _bad_leaf(arg0, arg1=0):
    return StatePredicate("bad", S.PRED_FIELD, arg0, arg1)


@pytest.mark.parametrize("pred,why", [
    (_bad_leaf(S.field_arg0(S.field_desc(2, 0, 4), S.CMP_EQ, False)), "node index"),
    (_bad_leaf(S.field_arg0(S.field_desc(1, 0, 0), S.CMP_EQ, False)), "width outside 1..32"),
    (_bad_leaf(S.field_arg0(S.field_desc(1, 0, 33), S.CMP_EQ, False)), "width outside 1..32"),
    (_bad_leaf(S.field_arg0(S.field_desc(1, 30, 4), S.CMP_EQ, False)), "straddles"),
    (_bad_leaf(S.field_arg0(S.field_desc(1, 192, 4), S.CMP_EQ, False)), "beyond the node"),
    (_bad_leaf(S.field_arg0(S.field_desc(1, 0, 4), 6, False)), "unknown comparison"),
    (_bad_leaf(S.field_arg0(S.field_desc(1, 0, 4), S.CMP_EQ, True), S.field_desc(1, 190, 4)), "right operand"),
    (_bad_leaf(S.field_arg0(S.field_desc(1, 0, 4), S.CMP_EQ, False), 1 << 32), "32 unsigned bits"),
])
def test_host_settings_refuse_a_bad_descriptor(pred, why):
    """resolve_settings / check_field_leaves (the engine's own checks) through the CPU baseline:
    PingPongIR(1 client) has 2 nodes of 6 words."""
    proto = PingPongIR(1, 3)
    with pytest.raises(subprocess.CalledProcessError) as e:
        cpu_baseline.run(proto, SearchSettings().addInvariant(pred), threads=1, table_log2=12)
    assert "field predicate" in e.value.stderr and why in e.value.stderr, e.value.stderr


def test_known_predicates_still_gate_unknown_ids():
    """Only DSL_PRED_FIELD passes without the protocol's consent."""
    with pytest.raises(subprocess.CalledProcessError) as e:
        cpu_baseline.run(PingPongIR(1, 3), SearchSettings().addInvariant(StatePredicate("x", 949)), threads=1,
                         table_log2=12)
    assert "not supported" in e.value.stderr
    r = cpu_baseline.run(PingPongIR(1, 3), SearchSettings().addPrune(CLIENTS_DONE), threads=1, table_log2=12)
    assert r["end"] == "SPACE_EXHAUSTED"


# ---- 3. the stand-alone host check ------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "hostcheck", "fieldcheck.cpp")


@pytest.fixture(scope="module", params=["plain", "ubsan"])
def fieldcheck(request):
    out = os.path.join(ROOT, "tests", "hostcheck", "_build", "fieldcheck_" + request.param)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    deps = [SRC] + [os.path.join(dp, f) for d in ("dslabs_amd/csrc", "include") for dp, _, fs in os.walk(os.path.join(ROOT, d))
                    for f in fs]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        flags = ["-O2"] if request.param == "plain" else \
            ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
        subprocess.run([HIPCC, "-std=c++17", "-Wno-unused-result", "-Wno-pass-failed"] + flags + ["-o", out, SRC], check=True)
    return out


def test_incremental_judge_agrees_on_every_successor(fieldcheck):
    """fieldcheck walks small BFSs of PingPongIR and MultiPaxosIR under field leaves (scalar, list
    element, sub-field, field-field, width-32 raw, negated, in combinators): the incremental verdict
    and an independent evaluation equal the full verdict on every successor; a field leaf judges
    some successors TERMINAL and some PRUNED. The ubsan build is the width-32 check."""
    p = subprocess.run([fieldcheck], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr
    rows = [json.loads(line) for line in p.stdout.splitlines()]
    total = rows[-1]
    assert total["total"] and total["ok"]
    assert total["judge_mismatch"] == 0 and total["ref_mismatch"] == 0 and total["errors"] == 0
    assert total["terminal"] > 0 and total["pruned"] > 0 and total["incremental"] > 0
    by = {r["scenario"]: r for r in rows[:-1]}
    assert {n[:2] for n in by} == {"pp", "mp"} and all(r["incremental"] > 0 for r in by.values())
    # the restated fixtures inside it: lab0_1c10p_goal is 84 states; the issue's implies-invariant 91
    assert by["pp_results_ok"]["judged"] + 1 == 84 and by["mp_implies"]["judged"] + 1 == 91
