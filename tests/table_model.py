"""A sequential model of the visited table in plain Python integers: the reference of
test_table_layout.py and test_gpu_table_kernels.py.

Written from the layout's description (csrc/fingerprint.hpp, "A table of 2^b buckets ..."), not
from its code. A fingerprint is the pair (hi, lo) of 64-bit words.

  * A table has 2^b buckets of 8 slots. The home bucket is lo's low b bits, the first slot in it
    hi's top 3 bits. A key is probed slot by slot from its home slot, through the end of the table
    to slot 0, and no further than the end of the bucket 7 past its home bucket.
  * A slot word: bit 0 = 1; bits 1-3 = the displacement d of the slot's bucket from the home
    bucket; then, with g = 32 - b0 (b0 = log2 of the search's first table), bits [4, 4 + g) =
    lo[b0, 32); above them hi's own bits [4 + g, 64).
  * So a word and its place pin lo[0, 32) and hi[4 + g, 64): 60 + b0 bits.
"""
KEY_BITS = 32   # home-bucket bits of the largest table
MAX_DISP = 7    # buckets a key may sit past its home bucket
M64 = (1 << 64) - 1

NEW, EXISTS, FULL = 0, 1, 2


def pinned(fp, b0):
    """The 60 + b0 bits that identify a state to the table, as a tuple."""
    hi, lo = fp
    g = KEY_BITS - b0
    return (lo & ((1 << KEY_BITS) - 1), hi >> (4 + g))


def pinned_positions(b0):
    """The pinned bit positions: ("lo" | "hi", bit)."""
    g = KEY_BITS - b0
    return {("lo", k) for k in range(KEY_BITS)} | {("hi", k) for k in range(4 + g, 64)}


def home(fp, b):
    """The home slot in a table of 2^b buckets."""
    hi, lo = fp
    return ((lo & ((1 << b) - 1)) << 3) | (hi >> 61)


def key0(fp, b0):
    """The slot word at displacement 0."""
    hi, lo = fp
    g = KEY_BITS - b0
    return ((hi >> (4 + g)) << (4 + g)) | (((lo >> b0) & ((1 << g) - 1)) << 4) | 1


def capacity(start_slot):
    """Slots a key may use: from its start slot to the end of the bucket MAX_DISP past its home."""
    return 8 * (MAX_DISP + 1) - start_slot


def rehome(b, b0, b2, i, v):
    """The home slot, in a table of 2^b2 buckets, of word v found at slot i of one of 2^b."""
    d = (v >> 1) & 7
    hb = ((i >> 3) - d) % (1 << b)
    g = KEY_BITS - b0
    lo_b0_32 = (v >> 4) & ((1 << g) - 1)  # lo[b0, 32)
    lo_b_32 = lo_b0_32 >> (b - b0)        # lo[b, 32)
    return (((hb | (lo_b_32 << b)) & ((1 << b2) - 1)) << 3) | (v >> 61)


class TableModel:
    def __init__(self, b, b0):
        assert 0 <= b0 <= b <= KEY_BITS
        self.b, self.b0 = b, b0
        self.slots = {}  # slot index -> word (a zero slot is absent)

    @property
    def nslots(self):
        return 8 << self.b

    def _place(self, h, base):
        """Walks the probe sequence from home slot h; base = the word without its displacement."""
        i = h
        for _ in range(capacity(h & 7)):
            d = ((i >> 3) - (h >> 3)) % (1 << self.b)
            if d > MAX_DISP:  # a table of fewer than 8 buckets: the walk came round
                break
            word = base | (d << 1)
            old = self.slots.get(i)
            if old is None:
                self.slots[i] = word
                return NEW
            if old == word:
                return EXISTS
            i = (i + 1) % self.nslots
        return FULL

    def insert(self, fp):
        return self._place(home(fp, self.b), key0(fp, self.b0))

    def rehash(self, b2):
        """Every key into a fresh table of 2^b2 buckets; returns (table, keys that found no slot)."""
        to = TableModel(b2, self.b0)
        bad = 0
        for i in sorted(self.slots):
            v = self.slots[i]
            bad += to._place(rehome(self.b, self.b0, b2, i, v), v & ~0xE & M64) == FULL
        return to, bad

    def key_multiset(self):
        return sorted(v & ~0xE & M64 for v in self.slots.values())


def check_slots(words, b, b0, identities):
    """The slot invariants of a dumped table (words: one per slot) against the fingerprints that
    were inserted and not refused (one per distinct pinned value). Raises AssertionError."""
    nb = 1 << b
    assert len(words) == 8 * nb
    want = {}
    for fp in identities:
        want.setdefault((home(fp, b), key0(fp, b0)), []).append(fp)
    assert all(len(v) == 1 for v in want.values()), "identities are not distinct"
    seen = set()
    for i, v in enumerate(words):
        if not v:
            continue
        assert v & 1, (i, hex(v))
        d = (v >> 1) & 7
        hb = ((i >> 3) - d) % nb
        h = (hb << 3) | (v >> 61)
        # at or after the home slot in probe order: in its home bucket, not before the start slot
        assert d > 0 or (i & 7) >= (v >> 61), (i, hex(v))
        j = h
        while j != i:  # no empty slot between the home slot and the key
            assert words[j], (i, hex(v), j)
            j = (j + 1) % (8 * nb)
        ident = (h, v & ~0xE & M64)
        assert ident in want, (i, hex(v))
        assert ident not in seen, (i, hex(v))
        seen.add(ident)
    assert len(seen) == len(want), (len(seen), len(want))
