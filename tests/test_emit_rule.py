"""The mask rule of the row emitter (dslabs_amd/csrc/nodestate.hpp: delta_new_slots,
emit_row_masked -- what wave_emit executes for a protocol of at most 64 records) against the rank
rule (emit_row, which test_hostcheck holds against materialize()), on the CPU.

tests/hostcheck/emitcheck.cpp walks the explored successors of small fixtures whose per-depth
vectors are in tests/golden/ and compares, on every successor, header and live records of the two
rows and the mask with creator_record's; then crafted rows. A test tool, never part of the product."""
import json
import os
import subprocess

import pytest

from dslabs_amd.protocols import MultiPaxos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "emitcheck.cpp")
BIN = os.path.join(ROOT, "tests", "hostcheck", "_build", "emitcheck")


@pytest.fixture(scope="module")
def emitcheck():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "tests", "hostcheck", "emit_cases.hpp")] + \
        [os.path.join(dp, f) for dp, _, fs in os.walk(os.path.join(ROOT, "dslabs_amd", "csrc")) for f in fs]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wno-unused-result", "-Wno-pass-failed", "-o", BIN,
                        SRC], check=True)
    return BIN


def run(bin_, args):
    out = subprocess.run([bin_] + [str(a) for a in args], check=True, capture_output=True, text=True, timeout=120)
    return json.loads(out.stdout)


def golden(name, key):
    with open(os.path.join(ROOT, "tests", "golden", name + ".json")) as f:
        return json.load(f)[key]["per_depth"]


_PB = [6, 2, 1, 2, 1, 0, 0, 3, 0, 0, 0, 5, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, -1]
# name: (emitcheck walk arguments (protocheck's), the golden per-depth vector the walk must follow,
#        whether some row keeps two or more sends)
WALKS = {
    "mp_3s2c_d6": ([5] + MultiPaxos(3, 2, "append-xy").params() + ["--", 1, 400, 300, "/", "/", 6],
                   golden("multipaxos", "mp_c5_d8")[:7], True),
    "sip_2p3a_d7": ([2, 2, 3, 0, "--", 101, 100, "/", "/", 7], golden("sipaxos", "sipaxos_2p3a_d9")[:8], True),
    # PB's handlers add at most one new record per step in this search: its rows count, its
    # multi-send rows are none
    "pb_2s1c_d10": (_PB + ["--", 1, "/", "/", 2, "500:4", 10], golden("pb", "pb_2s1c_d15")[:11], False),
    "minitest": ([7, "--", 700, "/", "/", -1], golden("event_census", "minitest"), True),
}


@pytest.fixture(scope="module")
def walks(emitcheck):
    return {name: run(emitcheck, ["walk"] + args) for name, (args, _, _) in WALKS.items()}


@pytest.mark.parametrize("name", sorted(WALKS))
def test_masked_row_equals_ranked_row_on_every_successor(walks, name):
    got = walks[name]
    assert got["per_depth"] == WALKS[name][1]  # the walk explored the fixture
    assert got["successors"] > 0
    assert got["mismatch"] == 0 and got["bad_bits"] == 0, got
    assert (got["multi_send_rows"] > 0) == WALKS[name][2]


def test_walks_cover_rows_with_several_kept_sends(walks):
    assert sum(w["multi_send_rows"] for w in walks.values()) > 0


# MultiPaxos (12 sends, 64 records of 8 bytes), PB (3 sends), SIPaxos (48 records of 4 bytes),
# MiniTest (4 records, 2 sends), and the IR twins
@pytest.mark.parametrize("proto", [5, 6, 2, 7, 10, 11], ids=["multipaxos", "pb", "sipaxos", "minitest", "multipaxos_ir",
                                                             "pb_ir"])
def test_crafted_rows(emitcheck, proto):
    cases = {c["name"]: c for c in run(emitcheck, ["crafted", proto])["cases"]}
    need = {"n0", "full", "full_last_new", "below_all", "above_all", "one_gap", "keep_holes", "all_sends", "no_new",
            "node_first", "node_last", "equal_sends"}
    assert need <= set(cases)
    assert cases["n0"]["n"] == 0 and cases["n0"]["m"] > 0
    cap = {5: 64, 6: 64, 2: 48, 7: 4, 10: 64, 11: 64}[proto]
    assert cases["full"]["n"] + cases["full"]["m"] == cap
    assert cases["full_last_new"]["n"] + 1 == cap
    assert cases["equal_sends"]["equal_sends"] is True  # bad == 0 there: the collision was reported
    if proto in (5, 10):
        assert cases["keep_holes"]["m"] == 3  # keep bits 0, 9, 11
    for c in cases.values():
        assert c["bad"] == 0, c
