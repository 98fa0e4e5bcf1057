"""The visited table's layout functions (csrc/fingerprint.hpp: table_key0, table_home,
table_rehome) against tests/table_model.py, on the CPU: tests/devcheck/tablecheck's `layout`
operation calls the product's own functions and makes no GPU call. Every comparison is exact."""
import pytest

import table_model as tm
import tablecheck_util as tu
from tablecheck_util import Scenario

B0S = [4, 7, 17, 20, 32]


@pytest.fixture(scope="module")
def tablecheck():
    try:
        return tu.ensure_built()
    except RuntimeError as e:
        pytest.fail(str(e))


def flip(fp, word, bit):
    hi, lo = fp
    return (hi ^ (1 << bit), lo) if word == "hi" else (hi, lo ^ (1 << bit))


POSITIONS = [("lo", k) for k in range(64)] + [("hi", k) for k in range(64)]


def sizes_from(b0):
    return sorted({b0, min(b0 + 3, 32), min(b0 + 11, 32), 32})


def test_key_and_home_pin_exactly_60_plus_b0_bits(tablecheck, tmp_path):
    """One-bit flips at all 128 positions: (home, key0) changes if and only if the bit is in
    lo[0, 32) or hi[4 + g, 64). Where the home stays (lo[b, 32), hi[4 + g, 61)) only the key word
    separates the two states."""
    rng = tu.SplitMix64(11)
    cases = []  # (b0, b, base fp)
    for b0 in B0S:
        for b in sizes_from(b0):
            for _ in range(3):
                cases.append((b0, b, rng.fp()))
            cases.append((b0, b, (0, 0)))
            cases.append((b0, b, (tm.M64, tm.M64)))
    entries = []
    for b0, b, fp in cases:
        for f in [fp] + [flip(fp, w, k) for w, k in POSITIONS]:
            entries.append((b0, b, b, f[0], f[1], 0, 1))
    res = tu.run_cpu(tablecheck, Scenario().layout(entries), tmp_path)[0]
    key0, home = tu.hex_words(res["key0"]), tu.hex_words(res["home"])
    assert len(key0) == len(home) == len(entries)
    at = 0
    for b0, b, fp in cases:
        g = 32 - b0
        pinned = tm.pinned_positions(b0)
        assert len(pinned) == 60 + b0
        assert (home[at], key0[at]) == (tm.home(fp, b), tm.key0(fp, b0)), (b0, b, fp)
        assert key0[at] & 0xF == 1  # bit 0 set, no displacement yet
        for n, (w, k) in enumerate(POSITIONS, start=1):
            f = flip(fp, w, k)
            got = (home[at + n], key0[at + n])
            assert got == (tm.home(f, b), tm.key0(f, b0)), (b0, b, w, k)
            differs = got != (home[at], key0[at])
            assert differs == ((w, k) in pinned), (b0, b, w, k)
            assert differs == (tm.pinned(f, b0) != tm.pinned(fp, b0))
            home_stays = (w == "lo" and b <= k < 32) or (w == "hi" and 4 + g <= k < 61)
            if home_stays:
                assert home[at + n] == home[at] and key0[at + n] != key0[at], (b0, b, w, k)
            if w == "lo" and k >= 32:  # the packed route record drops these: they must be unpinned
                assert not differs
        at += 1 + len(POSITIONS)


def rehome_grid():
    grid = set()
    for b0 in B0S:
        bs = sizes_from(b0)
        for b in bs:
            for b2 in {b, min(b + 1, 32), min(b + 2, 32), min(b + 5, 32), 32}:
                grid.add((b0, b, b2))  # b2 = b: the only size b0 = 32 has
    return sorted(grid)


def test_rehome_recovers_the_home_in_every_larger_table(tablecheck, tmp_path):
    """A word placed d buckets past its home (d = 0..7, across the end of the table too) in a table
    of 2^b buckets: table_rehome gives table_home in the table of 2^b2 buckets."""
    rng = tu.SplitMix64(12)
    entries, want = [], []
    for b0, b, b2 in rehome_grid():
        nb = 1 << b
        for t in range(6):
            hi, lo = rng.fp()
            if t < 3:  # a home bucket among the last 8, so that home + d passes the end
                lo = (lo & ~(nb - 1)) | ((nb - 1 - rng.next() % min(8, nb)) & (nb - 1))
            fp = (hi, lo)
            h = tm.home(fp, b)
            for d in range(8):
                if d >= nb:
                    continue
                slot = rng.next() % 8 if d else (h & 7) + rng.next() % (8 - (h & 7))
                i = ((((h >> 3) + d) % nb) << 3) | slot
                v = tm.key0(fp, b0) | (d << 1)
                entries.append((b0, b, b2, hi, lo, i, v))
                want.append((tm.home(fp, b2), tm.rehome(b, b0, b2, i, v)))
    res = tu.run_cpu(tablecheck, Scenario().layout(entries), tmp_path)[0]
    rehome, home = tu.hex_words(res["rehome"]), tu.hex_words(res["home"])
    assert len(rehome) == len(entries) > 2000
    for e, r, h, (wh, wr) in zip(entries, rehome, home, want):
        assert wh == wr, e  # the model agrees with itself
        assert r == wh, (e, r, wh)
        if e[1] == e[2]:
            assert r == h


def test_model_capacity_and_wrap():
    assert [tm.capacity(s) for s in (0, 3, 7)] == [64, 61, 57]
    rng = tu.SplitMix64(13)
    for s, cap in ((0, 64), (3, 61), (7, 57)):
        t = tm.TableModel(7, 7)
        fps = tu.cluster(7, 7, 127, s, cap + 1, rng)
        assert [t.insert(f) for f in fps[:cap]] == [tm.NEW] * cap
        assert t.insert(fps[cap]) == tm.FULL and len(t.slots) == cap
        assert [t.insert(f) for f in fps[:cap]] == [tm.EXISTS] * cap
        # the last bucket from slot s, then buckets 0-6 whole: 56 slots past the wrap
        assert sorted(t.slots) == list(range(56)) + list(range(127 * 8 + s, 128 * 8))
        assert all((t.slots[i] >> 1) & 7 == ((i >> 3) + 1) % 128 for i in range(56))
        tm.check_slots([t.slots.get(i, 0) for i in range(t.nslots)], 7, 7, fps[:cap])


@pytest.mark.parametrize("b,b0", [(7, 7), (10, 7), (17, 17), (20, 17)])
def test_model_merges_exactly_the_unpinned_flips(b, b0):
    g = 32 - b0
    fp = tu.SplitMix64(14 + b).fp()
    for w, k in POSITIONS:
        t = tm.TableModel(b, b0)
        assert t.insert(fp) == tm.NEW
        unpinned = (w == "hi" and k < 4 + g) or (w == "lo" and k >= 32)
        assert t.insert(flip(fp, w, k)) == (tm.EXISTS if unpinned else tm.NEW), (w, k)


@pytest.mark.parametrize("path", [(7, 8), (7, 12), (9, 10)])
def test_model_rehash_loses_nothing(path):
    b, b2 = path
    fps = tu.distinct_fps(tu.SplitMix64(1), 4 << b, 7)
    t, direct = tm.TableModel(b, 7), tm.TableModel(b2, 7)
    assert all(t.insert(f) == tm.NEW for f in fps)
    assert all(direct.insert(f) == tm.NEW for f in fps)
    to, bad = t.rehash(b2)
    assert bad == 0 and len(to.slots) == len(fps)
    assert to.key_multiset() == direct.key_multiset()
    assert all(to.insert(f) == tm.EXISTS for f in fps)
    tm.check_slots([to.slots.get(i, 0) for i in range(to.nslots)], b2, 7, fps)
