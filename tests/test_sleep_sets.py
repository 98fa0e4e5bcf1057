"""The sleep-set rule of k_level (dslabs_amd/csrc/nodestate.hpp: creator_record, sleeping) on the
host: tests/hostcheck/sleepcheck.cpp runs a BFS over the shared transition functions that keeps
each state's recorded parent row, draws the recorded creator at random among a state's generators
(the device's race), and checks the commuting property behind every sleeping event."""
import ctypes
import json
import os
import subprocess
import tempfile

import pytest

import argmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "sleepcheck.cpp")
BIN = os.path.join(ROOT, "tests", "hostcheck", "_build", "sleepcheck")
SEEDS = 20


def _gold(fname, name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", fname + ".json")))[name]


def _with_depth(args, depth):
    args = list(args)
    if "--max-depth" in args:
        k = args.index("--max-depth")
        del args[k:k + 2]
    return args + ["--max-depth", str(depth)]


@pytest.fixture(scope="module")
def sleepcheck():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    deps = [SRC] + [os.path.join(dp, f) for dp, _, fs in os.walk(os.path.join(ROOT, "dslabs_amd", "csrc"))
                    for f in fs]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wno-unused-result", "-o", BIN, SRC], check=True)
    return BIN


_cache = {}


def run(bin_, args, seeds=SEEDS):
    """One sleepcheck run per distinct search, shared by the tests that read it."""
    key = (tuple(args), seeds)
    if key not in _cache:
        proto = argmap.protocol(args)
        s = argmap.settings(args, proto)
        st = proto.initial_state()
        blob = bytes(proto.desc()) + bytes(s._encode(st))
        assert len(blob) == ctypes.sizeof(type(proto.desc())) + ctypes.sizeof(type(s._encode(st)))
        with tempfile.NamedTemporaryFile("wb", suffix=".blob", delete=False) as f:
            f.write(blob)
        try:
            out = subprocess.run([bin_, f.name, str(seeds)], check=True, capture_output=True, text=True, timeout=600)
        finally:
            os.unlink(f.name)
        _cache[key] = json.loads(out.stdout)
    return _cache[key]


MP6 = _with_depth(_gold("multipaxos", "mp_c5_d8")["args"], 6)
SIP6 = _gold("sipaxos", "sipaxos_2p3a_d6")["args"]
PP = _gold("lab0", "lab0_1c10p_exhaustive")["args"]
VIOL = [a for a in _gold("multipaxos", "mp_expect_violation")["args"] if a != "--finish-level"]
# (args, the golden per-depth vector, whether the settings allow the rule)
SHAPES = {
    "mp_c5_d6": (MP6, _gold("multipaxos", "mp_c5_d8")["per_depth"][:7], True),
    "sipaxos_d6": (SIP6, _gold("sipaxos", "sipaxos_2p3a_d6")["per_depth"], True),
    # PingPong's network holds up to 120 records, more than the mask's 64 (and the exhaustive search prunes): off
    "pingpong": (PP, _gold("lab0", "lab0_1c10p_exhaustive")["per_depth"], False),
    "mp_expect_violation": (VIOL, _gold("multipaxos", "mp_expect_violation")["per_depth"], True),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_race_independence(sleepcheck, name):
    """Whichever generator is recorded as a state's creator, the search is the plain BFS: per-depth
    counts, states, successors and the end (level, verdict, predicate), over 20 seeds."""
    args, per_depth, on = SHAPES[name]
    r = run(sleepcheck, args)
    assert r["errors"] == 0
    assert r["plain"]["per_depth"] == per_depth
    assert r["seeds"] >= 20 and r["differing"] == 0, (r["plain"], r["last"])
    assert r["rule_on"] is on
    if on:
        assert r["slept_all_seeds"] > 0 and r["last"]["slept_unfiltered"] > 0
    else:
        assert r["slept_all_seeds"] == 0


def test_mp_c5_d6_shape(sleepcheck):
    r = run(sleepcheck, MP6)
    assert r["plain"]["states"] == 2448


def test_violation_ends_alike(sleepcheck):
    case = _gold("multipaxos", "mp_expect_violation")
    r = run(sleepcheck, VIOL)
    assert case["end"] == "INVARIANT_VIOLATED"
    for k in ("end_level", "verdict", "pred"):
        assert r["last"][k] == r["plain"][k]
    assert r["plain"]["end_level"] == len(case["per_depth"]) - 1 and r["plain"]["verdict"] != 0


@pytest.mark.parametrize("name", sorted(n for n in SHAPES if SHAPES[n][2]))
def test_commuting_property(sleepcheck, name):
    """Every sleeping event is enabled in the recorded parent G, has the same delta there, and
    G+E+Cr has the fingerprint of P+E; the new-record mask marks exactly the new records."""
    r = run(sleepcheck, SHAPES[name][0])
    assert r["slept_all_seeds"] > 0
    assert r["not_enabled"] == 0 and r["delta_differs"] == 0 and r["fp_differs"] == 0
    assert r["mask_mismatch"] == 0


@pytest.mark.parametrize("extra", [["--prune", "CLIENTS_DONE"], ["--partition", "server1,server2,client1|server3,client2"]],
                         ids=["prune", "dropped_links"])
def test_conditions_switch_the_rule_off(sleepcheck, extra):
    """A prune in the settings (a pruned state is not expanded) or a link that does not deliver:
    the rule is off, no event sleeps, and the search is the plain one."""
    r = run(sleepcheck, _with_depth(MP6, 5) + extra, seeds=2)
    assert r["rule_on"] is False
    assert r["slept_all_seeds"] == 0 and r["differing"] == 0 and r["errors"] == 0
