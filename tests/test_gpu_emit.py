"""The product's wave_emit (csrc/kernels.hpp) in isolation: tests/devcheck/emitcheck runs one 64-lane
wave per case on crafted parents and deltas (tests/hostcheck/emit_cases.hpp) -- parents in global
memory, parents and node words in LDS, and the latter with the new-record mask returned -- into a
buffer pre-filled with a sentinel, and restates every row with emit_row and creator_record on the
host. Every comparison is exact: header and records below the count equal, every word past the
count (and every row nobody owns) still the sentinel, the mask creator_record's, the collision flag
as expected. One fresh child process per protocol, under its own time limit; after a run that
failed, every later test of the module fails without starting another GPU process."""
import json
import subprocess

import pytest

pytestmark = pytest.mark.gpu

# protocol ids (include/dslabs_hip.h)
PROTOS = {"multipaxos": 5, "pb": 6, "sipaxos": 2, "minitest": 7, "pingpong_ir": 8}
# these keep the rank rule (nodestate.hpp: MaskEmit): PingPongIR holds 120 records, PB opts out
RANK_RULE = {"pingpong_ir", "pb"}
CRAFTED = {"n0", "full", "full_last_new", "below_all", "above_all", "one_gap", "keep_holes", "all_sends", "no_new",
           "node_first", "node_last", "equal_sends"}
WAVES = {"active_none": 0, "active_lane0": 1, "active_lane63": 1, "active_all64": 64, "active_odd": 32}
GLOBAL, LDS, LDS_MASK = 0, 1, 2


class Runner:
    def __init__(self, bin_):
        self.bin = bin_
        self.poisoned = None
        self.done = {}

    def run(self, proto, limit=60):
        if proto in self.done:
            return self.done[proto]
        assert self.poisoned is None, f"an earlier run of emitcheck failed ({self.poisoned}): no further GPU run"
        out = subprocess.run(["timeout", "-k", "10", str(limit), self.bin, str(PROTOS[proto])], capture_output=True,
                             text=True)
        if out.returncode != 0:
            self.poisoned = f"exit status {out.returncode}: {out.stderr.strip()[-400:]}"
            raise AssertionError(f"emitcheck failed, {self.poisoned}")
        self.done[proto] = json.loads(out.stdout)
        return self.done[proto]


@pytest.fixture(scope="module")
def runner():
    import __graft_entry__ as g
    try:
        return Runner(g.build_emitcheck())
    except RuntimeError as e:
        pytest.fail(str(e))


@pytest.mark.parametrize("proto", list(PROTOS))
def test_wave_emit_rows(runner, proto):
    res = runner.run(proto)
    masked = proto not in RANK_RULE
    assert res["masked"] is masked
    modes = (GLOBAL, LDS, LDS_MASK) if masked else (GLOBAL, LDS)
    by = {(c["name"], c["mode"]): c for c in res["cases"]}
    names = {n for n, _ in by}
    assert CRAFTED <= names and set(WAVES) <= names
    assert set(by) == {(n, m) for n in names for m in modes}
    for (name, mode), c in sorted(by.items()):
        assert c["header_bad"] == 0 and c["record_bad"] == 0 and c["sentinel_bad"] == 0 and c["mask_bad"] == 0, c
        assert c["collision"] == c["expect_collision"], c
        if name in WAVES:
            assert c["rows"] == WAVES[name], c
        else:
            assert c["rows"] == 1, c
    # two equal kept sends are reported by the mask rule whatever the protocol; the rank rule looks
    # only where the Sender does not (P::kSendsDistinct, which neither PingPongIR nor PB sets)
    for mode in modes:
        assert by[("equal_sends", mode)]["expect_collision"] == (1 if masked else 0)
        assert by[("n0", mode)]["expect_collision"] == 0
