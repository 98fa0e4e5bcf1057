"""The visited table's kernels in isolation: k_probe_remote, k_probe_slab, k_rehash,
k_route_headers and k_new_list, launched by tests/devcheck/tablecheck (the product's own kernels
on the engine's grids) and judged against tests/table_model.py. Every comparison is exact.

Every run is one fresh child process under its own time limit. Under concurrency only which
duplicate wins depends on order, so the checks are order-free: one reply 1 per identity, the
counters, and the slot invariants of the dumped table (table_model.check_slots). A test with a
table runs with load_first 0 and 1 and wants the same answers from both. After a run that ended by
a signal, an abort, its time limit or an error, every later test of the module fails without
starting another GPU process (tablecheck_util.GpuRunner)."""
import numpy as np
import pytest

import table_model as tm
import tablecheck_util as tu
from tablecheck_util import Scenario, SplitMix64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runner():
    try:
        return tu.GpuRunner(tu.ensure_built())
    except RuntimeError as e:
        pytest.fail(str(e))


def replies(res):
    return np.frombuffer(bytes.fromhex(res["reply"]), dtype=np.uint8)


def dump_words(res):
    return tu.hex_words(res["slots"])


def model_fits(fps, b, b0):
    """The model's answers for the list in order; the tests want no FULL among them."""
    t = tm.TableModel(b, b0)
    ans = [t.insert(f) for f in fps]
    assert tm.FULL not in ans, "the model itself runs out of room: pick other seeds, do not filter"
    return t, ans


def with_unpinned_noise(fp, b0, rng):
    """The same identity, other unpinned bits: hi[0, 4 + g) and lo[32, 64)."""
    hi, lo = fp
    g = 32 - b0
    return (hi ^ (rng.next() & ((1 << (4 + g)) - 1)), lo ^ (rng.next() & (((1 << 32) - 1) << 32)))


# ---- random fill ---------------------------------------------------------------------------------

@pytest.mark.parametrize("b,b0", [(7, 7), (9, 7), (12, 12)])
def test_random_fill(runner, tmp_path, b, b0):
    fps = tu.distinct_fps(SplitMix64(1), 4 << b, b0)
    model_fits(fps, b, b0)
    keys = []
    for lf in (0, 1):
        r = runner.run(Scenario().table(b, b0, lf).probe_remote(fps).probe_remote(fps).dump(), tmp_path)
        assert replies(r[1]).tolist() == [1] * len(fps)
        assert (r[1]["new_states"], r[1]["err_table"]) == (len(fps), 0)
        assert replies(r[2]).tolist() == [0] * len(fps)
        assert (r[2]["new_states"], r[2]["err_table"]) == (0, 0)
        words = dump_words(r[3])
        tm.check_slots(words, b, b0, fps)
        keys.append(sorted(w & ~0xE for w in words if w))
    assert keys[0] == keys[1]


# ---- races ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["adjacent", "strided"])
def test_races_for_one_slot(runner, tmp_path, order):
    """4096 identities, 64 copies each that differ in unpinned bits only: adjacent (a whole wave
    races for one slot) or 4096 records apart (the copies fall in different workgroups)."""
    b = b0 = 12
    n, copies = 4096, 64
    rng = SplitMix64(2)
    ids = tu.distinct_fps(rng, n, b0)
    model_fits(ids, b, b0)
    recs = [[with_unpinned_noise(f, b0, rng) for _ in range(copies)] for f in ids]
    assert all(tm.pinned(c, b0) == tm.pinned(f, b0) for f, cs in zip(ids, recs) for c in cs[:2])
    if order == "adjacent":
        flat = [c for cs in recs for c in cs]
        ident = np.repeat(np.arange(n), copies)
    else:
        flat = [recs[i][c] for c in range(copies) for i in range(n)]
        ident = np.tile(np.arange(n), copies)
    for lf in (0, 1):
        r = runner.run(Scenario().table(b, b0, lf).probe_remote(flat).dump(), tmp_path)
        rep = replies(r[1])
        assert set(rep.tolist()) <= {0, 1}
        assert np.bincount(ident, weights=rep, minlength=n).tolist() == [1.0] * n
        assert (r[1]["new_states"], r[1]["err_table"]) == (n, 0)
        words = dump_words(r[2])
        assert sum(1 for w in words if w) == n
        tm.check_slots(words, b, b0, ids)


# ---- cluster and wrap ----------------------------------------------------------------------------

@pytest.mark.parametrize("bucket", [127, 61], ids=["last_bucket", "middle_bucket"])
def test_full_cluster_and_the_key_past_it(runner, tmp_path, bucket):
    b = b0 = 7
    nslots = 8 << b
    rng = SplitMix64(3 + bucket)
    groups = {s: tu.cluster(b, b0, bucket, s, 64 - s + 1, rng) for s in (0, 3, 7)}
    for s, fps in groups.items():  # the model: 64 - s fit, the next one does not
        t = tm.TableModel(b, b0)
        assert [t.insert(f) for f in fps] == [tm.NEW] * (64 - s) + [tm.FULL]
    for lf in (0, 1):
        sc = Scenario()
        for s in (0, 3, 7):
            fps = groups[s]
            sc.table(b, b0, lf).probe_remote(fps[:-1]).dump().probe_remote(fps[-1:]).dump().probe_remote(fps[:-1])
        r = runner.run(sc, tmp_path)
        for k, s in enumerate((0, 3, 7)):
            fps, (_, fill, d1, extra, d2, again) = groups[s], r[6 * k:6 * k + 6]
            cap = 64 - s
            assert replies(fill).tolist() == [1] * cap
            assert (fill["new_states"], fill["err_table"]) == (cap, 0)
            words = dump_words(d1)
            run = [(bucket * 8 + s + k2) % nslots for k2 in range(cap)]
            assert sorted(i for i, w in enumerate(words) if w) == sorted(run)
            for i in run:  # displacements 0-7, in bucket order from the home bucket
                assert (words[i] >> 1) & 7 == ((i >> 3) - bucket) % (1 << b) <= 7
                assert words[i] >> 61 == s
            if bucket == 127:  # the last bucket from slot s, then buckets 0-6 whole
                assert sorted(run) == list(range(56)) + list(range(127 * 8 + s, 128 * 8))
            tm.check_slots(words, b, b0, fps[:-1])
            assert replies(extra).tolist() == [0]
            assert (extra["new_states"], extra["err_table"]) == (0, 1)
            assert dump_words(d2) == words
            assert replies(again).tolist() == [0] * cap
            assert (again["new_states"], again["err_table"]) == (0, 0)


# ---- key discrimination --------------------------------------------------------------------------

@pytest.mark.parametrize("b,b0", [(7, 7), (10, 7), (12, 12)])
def test_key_word_alone_separates_states_of_one_home(runner, tmp_path, b, b0):
    """Pairs that differ in one bit which leaves the home unchanged: a pinned bit gives two new
    states, an unpinned one gives one."""
    g = 32 - b0
    rng = SplitMix64(4 + b)
    positions = [("lo", k) for k in range(b, 64)] + [("hi", k) for k in range(61)]
    bases = tu.distinct_fps(rng, len(positions), b0)
    pinned = tm.pinned_positions(b0)
    recs, want = [], []
    for fp, (w, k) in zip(bases, positions):
        hi, lo = fp
        other = (hi ^ (1 << k), lo) if w == "hi" else (hi, lo ^ (1 << k))
        assert tm.home(other, b) == tm.home(fp, b)
        recs += [fp, other]
        want.append(2 if (w, k) in pinned else 1)
    assert want.count(1) == 32 + 4 + g and want.count(2) == (32 - b) + (61 - 4 - g)
    t, ans = model_fits(recs, b, b0)
    assert [2 - ans[2 * i + 1] for i in range(len(positions))] == want  # the model agrees
    for lf in (0, 1):
        r = runner.run(Scenario().table(b, b0, lf).probe_remote(recs).dump(), tmp_path)
        rep = replies(r[1])
        assert set(rep.tolist()) <= {0, 1}
        got = (rep[0::2] + rep[1::2]).tolist()
        assert got == want, [(p, x, y) for p, x, y in zip(positions, got, want) if x != y]
        assert (r[1]["new_states"], r[1]["err_table"]) == (sum(want), 0)
        tm.check_slots(dump_words(r[2]), b, b0, [recs[2 * i + j] for i, n in enumerate(want) for j in range(n)])


# ---- rehash --------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", [(8, 9), (12,), (9, 10)], ids=["7-8-9", "7-12", "7-9-10"])
def test_rehash_keeps_every_key(runner, tmp_path, path):
    """A half-full table of 2^7 buckets with a cluster that wraps past its end, grown along `path`
    (b0 stays 7): several doublings at once, and rehashes from a table larger than the first."""
    b0 = 7
    rng = SplitMix64(5)
    # Near a cluster, which key finds no room depends on the order (a key may use only the slots
    # up to 7 buckets past its home, and the keys homed further on take them first if they come
    # first). So the cluster goes in by a launch of its own (24 keys of one home fit in any order),
    # and the model must place the rest after it in the list's order and in the reverse order.
    # The cluster's keys share lo[0, 12): their home is the last bucket of every table on the
    # path, so each rehash has to displace them across its own wrap again.
    wrapped = tu.cluster(12, b0, 4095, 3, 24, rng)
    rest = tu.distinct_fps(rng, 512 - len(wrapped), b0)
    fps = wrapped + rest
    assert len({tm.pinned(f, b0) for f in fps}) == len(fps)
    model_fits(wrapped + rest[::-1], 7, b0)
    t, _ = model_fits(fps, 7, b0)
    assert any(i < 56 and (w >> 1) & 7 for i, w in t.slots.items())  # keys displaced across the wrap
    fresh = tu.distinct_fps(SplitMix64(6), 300, b0)
    assert not {tm.pinned(f, b0) for f in fresh} & {tm.pinned(f, b0) for f in fps}
    want_keys = t.key_multiset()
    for b2 in path:
        direct, _ = model_fits(fps, b2, b0)
        assert direct.key_multiset() == want_keys
        t, bad = t.rehash(b2)
        assert bad == 0 and t.key_multiset() == want_keys
        assert sum(1 for i, w in t.slots.items() if i < 56 and (w >> 1) & 7) >= 16
    model_fits(fps + fresh, path[-1], b0)
    for lf in (0, 1):
        sc = Scenario().table(7, b0, lf).probe_remote(wrapped).probe_remote(rest).dump()
        for b2 in path:
            sc.rehash(b2).dump().probe_remote(fps)
        sc.probe_remote(fresh).dump()
        r = runner.run(sc, tmp_path)
        for fill, part in ((r[1], wrapped), (r[2], rest)):
            assert (fill["new_states"], fill["err_table"]) == (len(part), 0)
            assert replies(fill).tolist() == [1] * len(part)
        tm.check_slots(dump_words(r[3]), 7, b0, fps)
        for k, b2 in enumerate(path):
            re, dump, again = r[4 + 3 * k:7 + 3 * k]
            assert (re["err"], re["b"]) == (0, b2)
            words = dump_words(dump)
            assert sum(1 for w in words if w) == len(fps)
            tm.check_slots(words, b2, b0, fps)
            assert sorted(w & ~0xE for w in words if w) == want_keys
            assert replies(again).tolist() == [0] * len(fps)
            assert (again["new_states"], again["err_table"]) == (0, 0)
        new, last = r[-2:]
        assert replies(new).tolist() == [1] * len(fresh)
        assert (new["new_states"], new["err_table"]) == (len(fresh), 0)
        tm.check_slots(dump_words(last), path[-1], b0, fps + fresh)


# ---- slabs ---------------------------------------------------------------------------------------

CS = 70
SIZES = [0, 1, 63, 64, 65, CS, CS + 9]


class Regions:
    """The routed regions of one shard in both layouts, as flat word arrays."""

    def __init__(self, W, cs):
        self.W, self.cs = W, cs
        self.cap_fp, self.cap_pk = tu.region_caps(cs)
        self.key = [0] * (2 * W * self.cap_fp)
        self.pk = [0] * (W * self.cap_pk)

    def rec_index(self, q, j):
        """A record's index in its region: 16-byte layout (and the replies'), packed layout."""
        return tu.ROUTE_HDR + q * self.cs + j, tu.PK_HDR + q * self.cs + j

    def header(self, region, q, count):
        self.key[2 * region * self.cap_fp + q] = count
        self.pk[region * self.cap_pk + 2 * q] = count & 0xFFFFFFFF
        self.pk[region * self.cap_pk + 2 * q + 1] = count >> 32

    def record(self, region, q, j, fp):
        hi, lo = fp
        i16, i12 = self.rec_index(q, j)
        k = 2 * (region * self.cap_fp + i16)
        self.key[k], self.key[k + 1] = hi, lo  # struct Fp {hi, lo}
        p = region * self.cap_pk + tu.PK_WORDS * i12
        # as k_level packs a routed record: lo[0, 32), then hi's two halves
        self.pk[p], self.pk[p + 1], self.pk[p + 2] = lo & 0xFFFFFFFF, hi & 0xFFFFFFFF, hi >> 32

    def fill(self, region, count, fps):
        """Every sub-slab of a region full of records from the iterator, all headers `count`."""
        for q in range(tu.ROUTE_SEGS):
            self.header(region, q, count)
            for j in range(self.cs):
                self.record(region, q, j, next(fps))


def poison_regions(W, cs, b0, rng):
    """Regions no probe may read: full headers, records of identities that are nobody's."""
    R = Regions(W, cs)
    fps = iter(tu.distinct_fps(rng, W * tu.ROUTE_SEGS * cs, b0))
    for d in range(W):
        R.fill(d, cs, fps)
    return R


@pytest.mark.parametrize("me", [0, 1])
def test_slab_probe_matches_remote_probe_in_both_layouts(runner, tmp_path, me):
    W, b, b0 = 2, 9, 7
    rng = SplitMix64(7 + me)
    pool = tu.distinct_fps(rng, 1000, b0)
    counts = {(s, q): SIZES[rng.next() % len(SIZES)] for s in range(W) for q in range(tu.ROUTE_SEGS)}
    for k, c in enumerate(SIZES):  # every size at least once per source
        counts[(0, 3 * k)] = counts[(1, 3 * k + 1)] = c
    # what this shard routed (out: its own region is read, the other is not) and received (in:
    # the other source's region is read, its own index is not)
    poison = poison_regions(W, CS, b0, SplitMix64(70))
    out16, in16 = Regions(W, CS), Regions(W, CS)
    out16.key, out16.pk, in16.key, in16.pk = list(poison.key), list(poison.pk), list(poison.key), list(poison.pk)
    records = {}  # (source, reply index in its region) -> fingerprint
    for (s, q), c in sorted(counts.items()):
        R, region = (out16, me) if s == me else (in16, s)
        R.header(region, q, c)  # the raw count: past cs it is clipped by the reader
        for j in range(min(c, CS)):
            fp = with_unpinned_noise(pool[rng.next() % len(pool)], b0, rng)
            R.record(region, q, j, fp)
            records[(s, R.rec_index(q, j)[0])] = fp
    flat = [records[k] for k in sorted(records)]
    idents = {tm.pinned(f, b0): f for f in flat}
    by_source = [{tm.pinned(f, b0) for (s, _), f in records.items() if s == src} for src in range(W)]
    assert len(flat) > len(idents) + 1000 and len(by_source[0] & by_source[1]) > 100  # duplicates across the sources
    model_fits(list(idents.values()), b, b0)
    cap = out16.cap_fp

    def judge_slab(res, with_reply):
        rep_out = np.frombuffer(bytes.fromhex(res["reply"]), dtype=np.uint8)
        rep_in = np.frombuffer(bytes.fromhex(res["self_reply"]), dtype=np.uint8)
        assert len(rep_out) == len(rep_in) == W * cap
        assert (res["new_states"], res["err_table"]) == (len(idents), 0)
        touched = np.zeros((2, W * cap), dtype=bool)
        ones = {}
        for (s, i), fp in records.items():
            arr, at = (1, me * cap + i) if s == me else (0, s * cap + i)
            touched[arr, at] = True
            v = int((rep_in if s == me else rep_out)[at])
            if not with_reply:
                continue
            assert v in (0, 1), (s, i, v)
            ones[tm.pinned(fp, b0)] = ones.get(tm.pinned(fp, b0), 0) + v
        if with_reply:
            assert set(ones.values()) == {1} and len(ones) == len(idents)
        else:
            touched[:] = False
        # the headers, the bytes past min(count, cs) and the regions nobody answers keep 0xAA
        assert (rep_out[~touched[0]] == 0xAA).all() and (rep_in[~touched[1]] == 0xAA).all()

    for lf in (0, 1):
        sc = Scenario().table(b, b0, lf).probe_remote(flat).dump()
        sc.table(b, b0, lf).slab_load(W, me, CS, out16.key, in16.key, poison.pk, poison.pk).probe_slab(0, 1).dump()
        sc.table(b, b0, lf).slab_load(W, me, CS, poison.key, poison.key, out16.pk, in16.pk).probe_slab(1, 1).dump()
        sc.table(b, b0, lf).probe_slab(1, 0).dump()
        sc.table(b, b0, lf).slab_load(W, me, CS, out16.key, in16.key, poison.pk, poison.pk).probe_slab(0, 0).dump()
        r = runner.run(sc, tmp_path)
        rep = replies(r[1])
        assert (r[1]["new_states"], r[1]["err_table"]) == (len(idents), 0) and int(rep.sum()) == len(idents)
        want = sorted(w & ~0xE for w in dump_words(r[2]) if w)
        tm.check_slots(dump_words(r[2]), b, b0, list(idents.values()))
        for probe, dump, with_reply in ((r[5], r[6], 1), (r[9], r[10], 1), (r[12], r[13], 0), (r[16], r[17], 0)):
            judge_slab(probe, with_reply)
            words = dump_words(dump)
            tm.check_slots(words, b, b0, list(idents.values()))
            assert sorted(w & ~0xE for w in words if w) == want


# ---- headers -------------------------------------------------------------------------------------

@pytest.mark.parametrize("me", [0, 1])
def test_route_headers_are_what_the_slab_probe_reads(runner, tmp_path, me):
    W, b, b0 = 2, 12, 7
    rng = SplitMix64(8 + me)
    big = [CS + 1, CS + 9, (1 << 32) + 5, (1 << 40)]
    draw = lambda: (SIZES + big)[rng.next() % (len(SIZES) + len(big))]  # noqa: E731
    sent = [draw() for _ in range(W * tu.ROUTE_SEGS)]      # this shard's own route counters
    received = [draw() for _ in range(W * tu.ROUTE_SEGS)]  # the counters behind the regions it received
    for k, c in enumerate(SIZES + big):
        sent[me * tu.ROUTE_SEGS + k] = received[(1 - me) * tu.ROUTE_SEGS + 2 * k] = c
    clip = lambda cs: [min(c, CS) for c in cs]  # noqa: E731
    # every record place holds an identity of its own; the headers start as garbage
    out_r, in_r = Regions(W, CS), Regions(W, CS)
    fps = tu.distinct_fps(rng, 2 * W * tu.ROUTE_SEGS * CS, b0)
    it = iter(fps)
    garbage = 0x5555555555555555
    for R in (out_r, in_r):
        for d in range(W):
            R.fill(d, garbage, it)
    model_fits(fps, b, b0)
    cap = out_r.cap_fp
    pk_pairs = lambda cs: [w for c in cs for w in (c & 0xFFFFFFFF, c >> 32)]  # noqa: E731
    for lf in (0, 1):
        sc = Scenario().slab_load(W, me, CS, out_r.key, in_r.key, out_r.pk, in_r.pk)
        sc.route_headers(0, 0, 0, sent)      # no packed regions, no counter to zero
        sc.route_headers(0, 1, 1, sent)      # as the engine launches it
        sc.route_headers(1, 1, 0, received)  # the same kernel at the sources this shard hears from
        sc.table(b, b0, lf).probe_slab(0, 1).table(b, b0, lf).probe_slab(1, 1)
        r = runner.run(sc, tmp_path)
        h0, h1, h2 = r[1:4]
        assert h0["key_hdr"] == clip(sent) and h0["pk_hdr"] == pk_pairs([garbage] * (W * tu.ROUTE_SEGS))
        assert h0["zero_ctr"] != 0  # untouched without a pointer
        assert h1["key_hdr"] == clip(sent) and h1["pk_hdr"] == pk_pairs(clip(sent)) and h1["zero_ctr"] == 0
        assert h2["key_hdr"] == clip(received) and h2["pk_hdr"] == pk_pairs(clip(received)) and h2["zero_ctr"] != 0
        for probe in (r[5], r[7]):
            rep_out = np.frombuffer(bytes.fromhex(probe["reply"]), dtype=np.uint8)
            rep_in = np.frombuffer(bytes.fromhex(probe["self_reply"]), dtype=np.uint8)
            want_out = np.full(W * cap, 0xAA, dtype=np.uint8)
            want_in = np.full(W * cap, 0xAA, dtype=np.uint8)
            total = 0
            for s in range(W):
                for q in range(tu.ROUTE_SEGS):
                    n = min((sent if s == me else received)[s * tu.ROUTE_SEGS + q], CS)
                    at = s * cap + tu.ROUTE_HDR + q * CS
                    (want_in if s == me else want_out)[at:at + n] = 1  # every identity is new
                    total += n
            assert rep_out.tolist() == want_out.tolist() and rep_in.tolist() == want_in.tolist()
            assert (probe["new_states"], probe["err_table"]) == (total, 0)


# ---- new list ------------------------------------------------------------------------------------

GROUP_SIZES = [0, 1, 63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("density", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("dev", [1, 0], ids=["device_counts", "host_counts"])
def test_new_list_is_the_set_of_new_records(runner, tmp_path, dev, density):
    """k_new_list has no table: one run. The list as a set is the indexes whose reply byte is
    non-zero within the clipped counts; bytes outside them are noise that must not be listed."""
    W = tu.MAX_SHARDS
    rng = np.random.default_rng(9)
    if dev:
        cs = 2100
        cap = tu.ROUTE_HDR + tu.ROUTE_SEGS * cs
        groups = W * tu.ROUTE_SEGS
        rounds_at = tu.slab_gy(groups, cs) * tu.BLOCK
        assert cs > 2 * rounds_at  # three grid-stride rounds at the engine's gridDim.y
        sizes = GROUP_SIZES + [cs, cs + 9, (1 << 33) + 1, rounds_at, rounds_at + 1, 2 * rounds_at - 1]
        counters = [0] * groups
        for k, c in enumerate(sizes):
            counters[(37 * k + 5) % groups] = c
        counters[groups - 1] = 65
        spans = [((g // tu.ROUTE_SEGS) * cap + tu.ROUTE_HDR + (g % tu.ROUTE_SEGS) * cs, min(c, cs))
                 for g, c in enumerate(counters)]
    else:
        cs = 0
        cap = 70000
        rounds_at = tu.slab_gy(W, cap) * tu.BLOCK
        assert cap > 2 * rounds_at
        counters = GROUP_SIZES + [cap, rounds_at, rounds_at + 1, 2 * rounds_at + 77, 300, 0, 1, 64]
        assert len(counters) == W
        spans = [(g * cap, c) for g, c in enumerate(counters)]
    reply = np.where(rng.random(W * cap) < 0.5, rng.choice([1, 2, 0x80, 0xAA, 0xFF], W * cap), 0).astype(np.uint8)
    want = []
    for base, n in spans:
        if density == 0.0:
            reply[base:base + n] = 0
        elif density == 1.0:
            reply[base:base + n] = rng.choice([1, 2, 0x80, 0xFF], n)
        else:
            reply[base:base + n] = np.where(rng.random(n) < 0.2, rng.choice([1, 2, 0x80, 0xFF], n), 0)
        want += (base + np.flatnonzero(reply[base:base + n])).tolist()
    r = runner.run(Scenario().new_list(dev, W, cap, cs, counters, reply), tmp_path)[0]
    assert r["grid_y"] * tu.BLOCK == rounds_at
    assert r["n_list"] == len(r["list"]) == len(want) and r["stray"] == 0
    assert len(set(r["list"])) == len(r["list"])
    assert sorted(r["list"]) == want
