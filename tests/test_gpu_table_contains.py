"""table_contains (csrc/fingerprint.hpp), the read-only lookup of the event census, in isolation:
tests/devcheck/containscheck fills a zeroed table with the product's table_insert, asks
table_contains for inserted and never inserted keys, and dumps the table around the lookups. The
answers are compared with tests/table_model.py; every comparison is exact, with load_first 0 and 1.
One fresh child process per run, under its own time limit; after a run that failed, every later
test of the module fails without starting another GPU process."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import table_model as tm
import tablecheck_util as tu
from tablecheck_util import SplitMix64

pytestmark = pytest.mark.gpu
MAGIC = 0x3130534E49544E43


class Runner:
    def __init__(self, bin_):
        self.bin = bin_
        self.poisoned = None

    def run(self, tmp_path, b, b0, lf, fill, query, limit=60):
        assert self.poisoned is None, f"an earlier run of containscheck failed ({self.poisoned}): no further GPU run"
        path = os.path.join(str(tmp_path), "contains.bin")
        words = [MAGIC, b, b0, lf, len(fill), len(query)] + [w for fp in fill for w in fp] + [w for fp in query for w in fp]
        with open(path, "wb") as f:
            f.write(struct.pack("<%dQ" % len(words), *words))
        out = subprocess.run(["timeout", "-k", "10", str(limit), self.bin, path], capture_output=True, text=True)
        if out.returncode != 0:
            self.poisoned = f"exit status {out.returncode}: {out.stderr.strip()[-400:]}"
            raise AssertionError(f"containscheck failed, {self.poisoned}")
        r = json.loads(out.stdout)
        return (np.frombuffer(bytes.fromhex(r["insert"]), dtype=np.uint8).tolist(),
                np.frombuffer(bytes.fromhex(r["contains"]), dtype=np.uint8).tolist(), r["before"], r["after"])


@pytest.fixture(scope="module")
def runner():
    import __graft_entry__ as g
    try:
        return Runner(g.build_containscheck())
    except RuntimeError as e:
        pytest.fail(str(e))


def absent_keys(rng, n, b0, present):
    """n fingerprints whose pinned bits are no inserted key's."""
    taken = {tm.pinned(f, b0) for f in present}
    out = []
    while len(out) < n:
        f = rng.fp()
        if tm.pinned(f, b0) not in taken:
            out.append(f)
    return out


# b = 7: the smallest table the engine takes (2^10 slots)
@pytest.mark.parametrize("b,b0", [(7, 7), (9, 7), (12, 12)])
def test_random_fill(runner, tmp_path, b, b0):
    rng = SplitMix64(11)
    fps = tu.distinct_fps(rng, 4 << b, b0)  # half full
    model = tm.TableModel(b, b0)
    assert [model.insert(f) for f in fps] == [tm.NEW] * len(fps)
    absent = absent_keys(rng, len(fps), b0, fps)
    # an absent key that shares an inserted key's home slot walks that key's cluster to its end
    near = [((a[0] & ((1 << 61) - 1)) | (f[0] >> 61 << 61), (a[1] & ~((1 << b) - 1)) | (f[1] & ((1 << b) - 1)))
            for a, f in zip(absent[:256], fps)]
    near = [f for f in near if tm.pinned(f, b0) not in {tm.pinned(x, b0) for x in fps}]
    assert len(near) >= 250
    query = fps + absent + near
    for lf in (0, 1):
        ins, got, before, after = runner.run(tmp_path, b, b0, lf, fps, query)
        assert ins == [tm.NEW] * len(fps)
        assert got == [1] * len(fps) + [0] * (len(absent) + len(near))
        assert before == after  # the lookups stored nothing
        tm.check_slots(tu.hex_words(after), b, b0, fps)


def test_cluster_that_wraps_the_tables_end(runner, tmp_path):
    """40 keys sharing lo[0, 12), at home in the last bucket: they fill five buckets through the
    table's end into bucket 0."""
    b = b0 = 12
    rng = SplitMix64(12)
    fps = tu.cluster(b, b0, (1 << b) - 1, 2, 40, rng)
    absent = tu.cluster(b, b0, (1 << b) - 1, 2, 80, rng)[40:]
    absent = [f for f in absent if tm.pinned(f, b0) not in {tm.pinned(x, b0) for x in fps}]
    model = tm.TableModel(b, b0)
    assert [model.insert(f) for f in fps] == [tm.NEW] * 40
    assert min(model.slots) < 8 * 4 and max(model.slots) == (8 << b) - 1  # it did wrap
    for lf in (0, 1):
        ins, got, before, after = runner.run(tmp_path, b, b0, lf, fps, fps + absent)
        assert ins == [tm.NEW] * 40 and got == [1] * 40 + [0] * len(absent)
        assert before == after
        words = tu.hex_words(after)
        assert {i for i, w in enumerate(words) if w} == set(model.slots)


@pytest.mark.parametrize("bucket,s", [(127, 0), (61, 3)], ids=["last_bucket", "middle_bucket"])
def test_full_cluster_answers_false_and_terminates(runner, tmp_path, bucket, s):
    """A home slot whose whole probe range is taken: table_insert answers INS_FULL for one key more,
    and the lookup of that key walks the range to its end and answers false."""
    b = b0 = 7
    rng = SplitMix64(13 + bucket)
    fps = tu.cluster(b, b0, bucket, s, 64 - s + 1, rng)
    model = tm.TableModel(b, b0)
    assert [model.insert(f) for f in fps] == [tm.NEW] * (64 - s) + [tm.FULL]
    for lf in (0, 1):
        ins, got, before, after = runner.run(tmp_path, b, b0, lf, fps, fps)
        assert sorted(ins) == [tm.NEW] * (64 - s) + [tm.FULL]  # which key found no room depends on arrival order
        assert got == [0 if rc == tm.FULL else 1 for rc in ins]
        assert before == after and sum(1 for w in tu.hex_words(after) if w) == 64 - s


def test_empty_table_holds_nothing(runner, tmp_path):
    fps = tu.distinct_fps(SplitMix64(14), 300, 7)
    for lf in (0, 1):
        ins, got, before, after = runner.run(tmp_path, 7, 7, lf, [], fps)
        assert ins == [] and got == [0] * 300 and before == after and set(before) == {"0"}
