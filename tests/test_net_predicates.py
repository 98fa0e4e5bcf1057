"""User-written message predicates (MessagePattern.where -> DSL_PRED_NET / DSL_PRED_REC_COND), the
parts that need no GPU: the encoding against the C header's macros and the Java encoder, the
pattern API against the IR specs' record layouts, the Python-side errors, the host's refusals
(resolve_settings / check_net_leaves through tools/cpu_bfs.cpp), pb.json restated through the CPU
baseline, and the stand-alone host check (tests/hostcheck/netcheck.cpp), also built with
-fsanitize=undefined."""
import json
import os
import re
import subprocess

import pytest

import net_cases
from dslabs_amd import MessagePattern, SearchSettings, StatePredicate, _lib, allOf, message_matches, statePredicate
from dslabs_amd import search as S
from dslabs_amd.protocols import PB, AmoKVIR, MultiPaxosIR, PBIR, PingPongIR
from tools import cpu_baseline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "dslabs_amd", "csrc", "protocols", "gen")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- 1. encoding -----------------------------------------------------------------------------------
def test_record_condition_macros_round_trip(tmp_path):
    """The C header's DSL_REC_* macros and the Python encoding agree, both ways."""
    cases = [(0, 1, S.CMP_EQ), (63, 1, S.CMP_GT), (28, 11, S.CMP_LE), (32, 32, S.CMP_GE), (0, 32, S.CMP_NE),
             (65535, 63, S.CMP_LT)]
    src = ['#include <stdio.h>', '#include "dslabs_hip.h"', "int main(void) {"]
    for bit, width, cmp in cases:
        src.append(f"{{ int64_t a = DSL_REC_ARG0({bit}, {width}, {cmp});"
                   ' printf("%lld %d %d %d %d\\n", (long long)a, DSL_REC_ARG0_BIT(a), DSL_REC_ARG0_WIDTH(a),'
                   " DSL_REC_ARG0_CMP(a), (int)(((uint64_t)a & ~DSL_REC_ARG0_MASK) != 0)); }")
    src.append('printf("%d %d %d %d\\n", DSL_PRED_NET, DSL_PRED_REC_COND, DSL_MAX_NET_CONDS, DSL_MAX_NET_CONDS_TOTAL);'
               " return 0; }")
    c = tmp_path / "rec.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "rec"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    for (bit, width, cmp), line in zip(cases, lines):
        a, b2, w2, c2, stray = (int(x) for x in line.split())
        assert a == S.rec_arg0(bit, width, cmp) and (b2, w2, c2) == (bit, width, cmp) == S.rec_arg0_decode(a)
        assert not stray
    assert [int(x) for x in lines[-1].split()] == [S.PRED_NET, S.PRED_REC_COND, S.MAX_NET_CONDS, S.MAX_NET_CONDS_TOTAL]
    assert S.MAX_NET_CONDS >= 6  # type, from, to and three fields: hasViewReply(n, p, b) at one address


def test_java_encoder_matches_the_header():
    with open(os.path.join(ROOT, "java", "src", "dslabs", "framework", "testing", "search", "gpu",
                           "GpuPredicates.java")) as f:
        java = f.read()
    with open(os.path.join(ROOT, "include", "dslabs_hip.h")) as f:
        hdr = f.read()
    ids = {n: int(re.search(r"DSL_PRED_%s = (\d+)" % n, hdr).group(1)) for n in ("NET", "REC_COND")}
    assert ids == {"NET": S.PRED_NET, "REC_COND": S.PRED_REC_COND}
    ncond = int(re.search(r"#define DSL_MAX_NET_CONDS (\d+)", hdr).group(1))
    assert "NET = %d, REC_COND = %d, MAX_NET_CONDS = %d;" % (ids["NET"], ids["REC_COND"], ncond) in java
    assert "(long) bit | ((long) width << 16) | ((long) cmp << 32)" in java  # DSL_REC_ARG0
    assert int(re.search(r"#define DSL_ABI_VERSION (\d+)", hdr).group(1)) == 6 == _lib.DSL_ABI_VERSION


# ---- 2. the pattern API against the specs' record layouts ------------------------------------------------
def _conds(pred):
    return [(c.bit, c.width, c.cmp, c.const) for c in pred.conds]


def test_view_reply_pattern_is_what_the_generated_header_reads():
    pb = PBIR(2, 1, "putget")
    vr = pb.message("ViewReply")
    assert isinstance(vr, MessagePattern)
    p = vr.where(vr.field("num") >= 4)
    assert p.name == "contains ViewReply(num >= 4)" and p.pred_id == S.PRED_NET and not p.negated
    # the header's hasViewReply: rec_type(r) == 2 && ((r >> 0) & 15u) >= arg0, rec_type = r >> 60
    with open(os.path.join(GEN, "pb_ir.hpp")) as f:
        src = f.read()
    assert "rec_type(r) == 2 && (((int)((r >> 0) & 15u) >= (int)pr.arg0))" in src
    assert "int rec_type(Rec r) { return (int)(r >> 60); }" in src
    assert "int rec_from(Rec r) { return (int)((r >> 57) & 7); }" in src and "int rec_to(Rec r) { return (int)((r >> 54) & 7); }" in src
    assert _conds(p) == [(60, 4, S.CMP_EQ, 2), (0, 4, S.CMP_GE, 4)]
    exact = vr.where(vr.field("num") == 2, vr.field("p") == 1, vr.field("b") == 2)
    assert _conds(exact)[1:] == [(0, 4, S.CMP_EQ, 2), (4, 2, S.CMP_EQ, 1), (6, 2, S.CMP_EQ, 2)]
    assert exact.name == "contains ViewReply(num == 2, p == 1, b == 2)"
    to = pb.message("ViewReply", frm="viewserver", to="client1")
    assert _conds(to.where()) == [(60, 4, S.CMP_EQ, 2), (57, 3, S.CMP_EQ, 0), (54, 3, S.CMP_EQ, 3)]
    assert to.where().name == "contains ViewReply from viewserver to client1"
    assert net_cases.has_view_reply(pb, 1, 1, -1).conds[3].const == 0  # null backup


def test_patterns_of_the_other_protocols():
    mp = MultiPaxosIR(3, 2, "append-xy")
    p2a = mp.message("P2a", frm="server3")
    p = p2a.where(p2a.field("round") >= 2).negate()
    assert p.name == "¬(contains P2a from server3(round >= 2))" and p.negated
    assert _conds(p) == [(61, 3, S.CMP_EQ, 4), (58, 3, S.CMP_EQ, 2), (0, 4, S.CMP_GE, 2)]
    l3 = mp.message("P1b").field("l3")
    assert (l3.bit, l3.width) == (28, 11)  # across bit 32 of the 64-bit record
    dec = mp.message("Decision")
    assert _conds(dec.where(dec.field("slot") == 1)) == [(61, 3, S.CMP_EQ, 6), (0, 3, S.CMP_EQ, 1)]
    pp = PingPongIR(1, 10)
    pong = pp.message("PongReply")
    assert _conds(pong.where(pong.field("value") == 3)) == [(31, 1, S.CMP_EQ, 1), (0, 4, S.CMP_EQ, 3)]
    kv = AmoKVIR(2, "diffkey3")
    rep = kv.message("Reply", to="client2")
    assert _conds(rep.where(rep.field("seq") == 3)) == [(31, 1, S.CMP_EQ, 1), (27, 2, S.CMP_EQ, 2), (0, 2, S.CMP_EQ, 3)]
    # a hand-written protocol: raw bits (pb.hpp: type = m >> 60, view = m & 0xff)
    raw = PB(2, 1, "putget").raw_message("ViewReply")
    q = raw.where(raw.raw_field(60, 4) == 2, raw.raw_field(0, 4) >= 3)
    assert _conds(q) == [(60, 4, S.CMP_EQ, 2), (0, 4, S.CMP_GE, 3)]
    assert q.name == "contains ViewReply(bits[60:64] == 2, bits[0:4] >= 3)"


def test_combinators_and_the_c_abi_form():
    pb = PBIR(2, 1, "putget")
    vr = pb.message("ViewReply")
    a, b = vr.where(vr.field("num") >= 2), vr.where(vr.field("num") == 2, vr.field("p") == 1, vr.field("b") == 2)
    st = pb.initial_state()
    pool = []
    enc = a.negate()._encode(st, pool)
    assert (enc.pred_id, enc.negate, enc.arg0, enc.arg1) == (S.PRED_NET, 1, 0, 2)
    assert [(p.pred_id, p.negate, S.rec_arg0_decode(p.arg0), p.arg1) for p in pool] == \
        [(S.PRED_REC_COND, 0, (60, 4, S.CMP_EQ), 2), (S.PRED_REC_COND, 0, (0, 4, S.CMP_GE), 2)]
    tree = a.and_(b.negate())
    assert tree.name == "(contains ViewReply(num >= 2)) ∧ (¬(contains ViewReply(num == 2, p == 1, b == 2)))"
    pool = []
    enc = tree._encode(st, pool)
    assert enc.pred_id == S.PRED_AND
    left, right = pool[enc.arg0], pool[enc.arg1]
    assert (left.pred_id, left.arg1, right.pred_id, right.negate, right.arg1) == (S.PRED_NET, 2, S.PRED_NET, 1, 4)
    for leaf in (left, right):  # consecutive record conditions
        assert all(pool[leaf.arg0 + i].pred_id == S.PRED_REC_COND for i in range(leaf.arg1))
    named = statePredicate("view 2 is out", a)
    assert named.name == "view 2 is out" and named.conds == a.conds and named.negate().conds == a.conds
    for p in (a.or_(b), a.implies(b), allOf([a, b, pb.predicate("viewRepliesSent:2:1:2:server1")])):
        SearchSettings().addGoal(p)._encode(st)
    assert isinstance(a, StatePredicate)


def test_errors_are_raised_in_python():
    pb, mp = PBIR(2, 1, "putget"), MultiPaxosIR(3, 2)
    vr = pb.message("ViewReply")
    bad = [
        lambda: pb.message("ViewReplay"),                        # unknown message
        lambda: vr.field("viewNum"),                             # unknown field (the spec calls it num)
        lambda: pb.message("ViewReply", frm="server3"),          # unknown address (2 servers)
        lambda: pb.message("ViewReply", to="nobody"),
        lambda: pb.message("ViewReply", to=7),
        lambda: vr.field("num") >= 16,                           # a constant wider than the field
        lambda: vr.field("p") == 4,
        lambda: vr.field("num") == -1,
        lambda: pb.message("GetView").where(),                   # fine: the type alone ...
        lambda: PB().raw_message().where(),                      # ... but a raw pattern needs a condition
        lambda: PB().raw_message().raw_field(60, 5),             # raw fields: inside the record, 1..32 bits
        lambda: PB().raw_message().raw_field(0, 33),
        lambda: PB().raw_message().raw_field(0, 0),
        lambda: PB().raw_message().raw_field(-1, 4),
        lambda: PB().raw_message(rec_bits=32).raw_field(30, 4),
        lambda: PB().raw_message(rec_bits=48),
        lambda: PB().raw_message().field("num"),                 # a raw pattern has no named fields
        lambda: message_matches(pb.initial_state(), pb.predicate("hasViewReply:1")),
    ]
    raised = []
    for k, f in enumerate(bad):
        try:
            f()
            raised.append(False)
        except ValueError:
            raised.append(True)
    assert raised == [True] * 8 + [False] + [True] * 9
    with pytest.raises(TypeError):
        vr.field("num") == "1"
    with pytest.raises(TypeError):
        vr.where(S.RESULTS_OK)                                   # a state predicate is no record condition
    # too many conditions in one leaf: type + from + to + 6 > 8
    p1b = mp.message("P1b", frm="server1", to="server2")
    six = [p1b.field(n) >= 0 for n in ("round", "leader", "l1", "l2", "l3", "l4")]
    p1b.where(*six[:5])
    with pytest.raises(ValueError, match="conditions, at most 8"):
        p1b.where(*six)
    # ... and in all (32), and the pool shared with the combinators' operands (48)
    leaf = vr.where(vr.field("num") >= 1, vr.field("p") == 1, vr.field("b") == 2)  # 4 conditions
    with pytest.raises(ValueError, match="too many message conditions in one search"):
        s = SearchSettings()
        for _ in range(9):
            s.addGoal(leaf)
        s._encode(pb.initial_state())
    two = vr.where(vr.field("num") >= 1)
    with pytest.raises(ValueError, match="too many combinator operands and message conditions"):
        SearchSettings().addInvariant(allOf([two] * 13))._encode(pb.initial_state())  # 26 + 24 pool entries
    SearchSettings().addInvariant(allOf([two] * 12))._encode(pb.initial_state())      # 24 + 22


def test_records_and_message_matches_decode_the_state():
    """SearchState.records() / message_matches on initial states (dsl_init_state: host only)."""
    pp = PingPongIR(1, 10)
    st = pp.initial_state()
    ping = pp.message("PingRequest", frm="client1", to="pingserver")
    recs = st.records()
    assert recs == [(0 << 31) | (1 << 28) | (0 << 25) | 1]  # PingRequest(1) from node 1 to node 0
    assert message_matches(st, ping.where(ping.field("value") == 1)) == recs
    assert message_matches(st, ping.where(ping.field("value") == 2)) == []
    assert message_matches(st, pp.message("PongReply").where()) == []
    assert st.packed is None  # records() leaves the state alone
    pb = PBIR(2, 1, "putget")
    st = pb.initial_state()
    n = len(st.records())
    assert n >= 3 and st.records() == sorted(st.records())
    st.dropPendingMessages()  # the dropped records stay part of network()
    assert len(st.records()) == n and len(message_matches(st, pb.message("Ping").where())) == 2


# ---- 3. the host's refusals (resolve_settings / check_net_leaves) ------------------------------------------
class _Raw(StatePredicate):
    """A predicate encoded as given: `pred` after `pool_entries` were appended to the pool; a
    NET `pred` with arg0 None refers to the first appended entry."""

    def __init__(self, pred, pool_entries=()):
        super().__init__("raw", pred[0])
        self.pred, self.pool_entries = pred, list(pool_entries)

    def _encode(self, state, pool):
        first = len(pool)
        for e in self.pool_entries:
            pool.append(_lib.dsl_predicate(*e))
        pid, neg, a0, a1 = self.pred
        return _lib.dsl_predicate(pid, neg, first if a0 is None else a0, a1)


def _cond(bit=0, width=4, cmp=S.CMP_EQ, const=1, negate=0, extra=0):
    return (S.PRED_REC_COND, negate, S.rec_arg0(bit, width, cmp) | extra, const)


_GOOD = _cond()
REFUSALS = [
    (_Raw((S.PRED_NET, 0, None, 1), [_cond(extra=1 << 22)]), "arg0 has bits set outside"),
    (_Raw((S.PRED_NET, 0, None, 1), [_cond(extra=1 << 35)]), "arg0 has bits set outside"),
    (_Raw((S.PRED_NET, 0, None, 1), [_cond(negate=1)]), "negate set on a record condition"),
    (_Raw((S.PRED_NET, 0, None, 1), [_cond(cmp=6)]), "unknown comparison 6"),
    (_Raw((S.PRED_NET, 0, None, 1), [_cond(width=0)]), "width outside 1..32"),
    (_Raw((S.PRED_NET, 0, None, 1), [_cond(width=33)]), "width outside 1..32"),
    (_Raw((S.PRED_NET, 0, None, 1), [_cond(const=1 << 32)]), "arg1 does not fit in 32 unsigned bits"),
    (_Raw((S.PRED_NET, 0, None, 1), [_cond(const=-1)]), "arg1 does not fit in 32 unsigned bits"),
    (_Raw((S.PRED_NET, 0, None, 2), [_GOOD]), "condition range outside dsl_settings.pool"),
    (_Raw((S.PRED_NET, 0, -1, 1), [_GOOD]), "condition range outside dsl_settings.pool"),
    (_Raw((S.PRED_NET, 0, 40, 1), [_GOOD]), "condition range outside dsl_settings.pool"),
    (_Raw((S.PRED_NET, 0, None, 0), [_GOOD]), "conditions, outside 1..8"),
    (_Raw((S.PRED_NET, 0, None, 9), [_GOOD] * 9), "conditions, outside 1..8"),
    (_Raw((S.PRED_NET, 0, None, 2), [_GOOD, (S.PRED_FIELD, 0, S.field_arg0(S.field_desc(1, 0, 4), S.CMP_EQ, False), 1)]),
     "not a DSL_PRED_REC_COND"),
    (_Raw(_GOOD), "used as a predicate or a combinator operand"),
    (_Raw((S.PRED_OR, 0, None, 0), [_GOOD]), "used as a predicate or a combinator operand"),
    (_Raw((S.PRED_NET, 0, None, 1), [_cond(bit=30, width=4)]), "beyond the record's 32 bits"),  # check_net_leaves<P>
    (_Raw((S.PRED_NET, 0, None, 1), [_cond(bit=32, width=1)]), "beyond the record's 32 bits"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_host_settings_refuse_a_bad_network_leaf(k):
    """PingPongIR has 32-bit records."""
    pred, why = REFUSALS[k]
    with pytest.raises(subprocess.CalledProcessError) as e:
        cpu_baseline.run(PingPongIR(1, 3), SearchSettings().addInvariant(pred), threads=1, table_log2=12)
    assert "settings:" in e.value.stderr and why in e.value.stderr, e.value.stderr
    assert "not supported" not in e.value.stderr  # DSL_ERR_ARG, not DSL_ERR_UNKNOWN_PREDICATE


def test_host_settings_refuse_too_many_conditions_in_all(monkeypatch):
    monkeypatch.setattr(S, "MAX_NET_CONDS_TOTAL", 1000)  # past the Python-side check: the host's own
    five = _Raw((S.PRED_NET, 0, None, 8), [_GOOD] * 8)
    s = SearchSettings()
    for _ in range(5):  # 40 > DSL_MAX_NET_CONDS_TOTAL, 40 pool entries <= DSL_MAX_POOL
        s.addGoal(five)
    with pytest.raises(subprocess.CalledProcessError) as e:
        cpu_baseline.run(PingPongIR(1, 3), s, threads=1, table_log2=12)
    assert "more than 32 conditions in all" in e.value.stderr
    s = SearchSettings()
    for _ in range(4):
        s.addGoal(five)
    assert cpu_baseline.run(PingPongIR(1, 3), s, threads=1, table_log2=12)["end"] == "GOAL_FOUND"  # PingRequest(1) is there


def test_a_64_bit_record_takes_a_field_across_bit_32():
    mp = MultiPaxosIR(3, 2, "append-xy")
    s = SearchSettings().addInvariant(_Raw((S.PRED_NET, 1, None, 1), [_cond(bit=28, width=32, cmp=S.CMP_GT, const=0xFFFFFFFE)]))
    assert cpu_baseline.run(mp, s.maxDepth(3), threads=1, table_log2=16)["end"] == "SPACE_EXHAUSTED"
    with pytest.raises(subprocess.CalledProcessError) as e:
        cpu_baseline.run(mp, SearchSettings().addInvariant(_Raw((S.PRED_NET, 0, None, 1), [_cond(bit=40, width=25)])),
                         threads=1, table_log2=12)
    assert "beyond the record's 64 bits" in e.value.stderr


# ---- 4. pb.json restated through the CPU baseline ---------------------------------------------------------
def test_every_pb_case_is_restated():
    assert len(net_cases.CASES) == 7 and "pb_initview_search" in net_cases.CASES
    _, _, s = net_cases.case("pb_initview_search")
    ids = lambda p: [p.pred_id] if not p.operands else [i for o in p.operands for i in ids(o)]  # noqa: E731
    assert [ids(p) for p in s.prunes()] == [[S.PRED_NET], [S.PRED_NET, S.PRED_NET]]
    assert ids(s.goals()[0]) == [502, S.PRED_NET]  # viewRepliesSent stays a named predicate


@pytest.mark.parametrize("name", net_cases.CASES)
def test_cpu_judge_matches_pb_golden_with_message_predicates(name):
    gold, proto, settings = net_cases.case(name)
    r = cpu_baseline.run(proto, settings, threads=2, table_log2=20)
    assert r["end"] == gold["end"]
    assert r["per_depth"] == gold["per_depth"]
    assert r["states"] == gold["states"]
    if gold["terminal_depth"] >= 0:  # cpu_bfs finishes the terminal's level and stops
        assert len(r["per_depth"]) - 1 == gold["terminal_depth"]


# ---- 5. the stand-alone host check ------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "hostcheck", "netcheck.cpp")


def netcheck_build(kind):
    out = os.path.join(ROOT, "tests", "hostcheck", "_build", "netcheck_" + kind)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    deps = [SRC] + [os.path.join(dp, f) for d in ("dslabs_amd/csrc", "include") for dp, _, fs in os.walk(os.path.join(ROOT, d))
                    for f in fs]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        flags = ["-O2"] if kind == "plain" else \
            ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
        subprocess.run([HIPCC, "-std=c++17", "-Wno-unused-result", "-Wno-pass-failed"] + flags + ["-o", out, SRC], check=True)
    return out


def netcheck_rows(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr
    return [json.loads(line) for line in p.stdout.splitlines()]


@pytest.mark.parametrize("kind", ["plain", "ubsan"])
def test_incremental_judge_agrees_on_every_successor(kind):
    """netcheck walks small BFSs of PBIR, PB, MultiPaxosIR, PingPongIR and AmoKVIR under network
    leaves (single, negated, in and / or / implies; invariant, goal and prune; a dropped network):
    the incremental verdict and an independent evaluation equal the full verdict on every
    successor; new records flipped a leaf on some successors, and the leaf was skipped as
    unchanged on others. The ubsan build is the check of the width-32 mask and the 64-bit shift."""
    rows = netcheck_rows(netcheck_build(kind))
    total = rows[-1]
    assert total["total"] and total["ok"]
    assert total["judge_mismatch"] == 0 and total["ref_mismatch"] == 0 and total["errors"] == 0
    assert total["flips"] > 0 and total["skipped"] > 0
    assert total["terminal"] > 0 and total["pruned"] > 0 and total["incremental"] > 0
    by = {r["scenario"]: r for r in rows[:-1]}
    assert {n.split("_")[0] for n in by} == {"pbir", "pb", "mp", "pp", "kv"}
    assert all(r["incremental"] > 0 and r["flips"] > 0 and r["skipped"] > 0 for r in by.values())
    # the hand-written and the generated PB are one protocol: the same search over the dropped network
    strip = lambda r: {k: v for k, v in r.items() if k != "scenario"}  # noqa: E731
    assert strip(by["pb_dropped"]) == strip(by["pbir_dropped"])
