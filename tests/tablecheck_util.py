"""tests/devcheck/tablecheck: building it, writing its scenarios, running it, reading its answers.

The program executes; this module makes the inputs and the tests judge the outputs (table_model.py
is the reference)."""
import json
import os
import struct
import subprocess

import numpy as np

import table_model as tm

# csrc/kernels.hpp
ROUTE_SEGS = 32
ROUTE_HDR = ROUTE_SEGS // 2
PK_WORDS = 3
PK_HDR = (2 * ROUTE_SEGS + PK_WORDS - 1) // PK_WORDS
MAX_SHARDS = 16
BLOCK = 256
M64 = (1 << 64) - 1


class SplitMix64:
    """The fixed-seed 64-bit generator of the table tests."""

    def __init__(self, seed):
        self.x = seed & M64

    def next(self):
        self.x = (self.x + 0x9E3779B97F4A7C15) & M64
        z = self.x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def fp(self):
        hi = self.next()
        return (hi, self.next())


def distinct_fps(rng, n, b0):
    """n fingerprints, no two with the same pinned bits (nothing is filtered out of a test's
    records: a 2^-60 coincidence is redrawn here, before the test has its list)."""
    out, seen = [], set()
    while len(out) < n:
        fp = rng.fp()
        p = tm.pinned(fp, b0)
        if p not in seen:
            seen.add(p)
            out.append(fp)
    return out


def cluster(b, b0, bucket, s, n, rng):
    """n distinct identities whose home, in a table of 2^b buckets, is slot s of `bucket`."""
    out, seen = [], set()
    while len(out) < n:
        hi, lo = rng.fp()
        fp = ((hi & ((1 << 61) - 1)) | (s << 61), (lo & ~((1 << b) - 1)) | bucket)
        if tm.pinned(fp, b0) not in seen:
            seen.add(tm.pinned(fp, b0))
            out.append(fp)
    return out


def ensure_built():
    """The binary: __graft_entry__.build_devcheck rebuilds it when it is older than the kernels or
    its source, and raises where it cannot (the caller fails, it does not skip)."""
    import __graft_entry__ as g
    return g.build_devcheck()


class Scenario:
    """The operations of one run, in order (the format: tablecheck.hip)."""

    def __init__(self):
        self.parts = [struct.pack("<Q", 0x31304B48434C4254)]

    def _words(self, *w):
        self.parts.append(np.asarray(w, dtype=np.uint64).astype("<u8").tobytes())

    def _image(self, arr, dtype):
        raw = np.ascontiguousarray(np.asarray(arr, dtype=dtype)).astype(np.dtype(dtype).newbyteorder("<")).tobytes()
        self.parts.append(raw + b"\0" * (-len(raw) % 8))

    def table(self, b, b0, load_first):
        self._words(1, b, b0, load_first)
        return self

    def probe_remote(self, fps):
        self._words(2, len(fps))
        self._image([w for fp in fps for w in fp], np.uint64)
        return self

    def slab_load(self, W, me, cs, out_key, in_key, out_pk, in_pk):
        """out_key / in_key: W * cap_fp records {hi, lo} as flat arrays of 64-bit words (a header
        word is a count); out_pk / in_pk: W * cap_pk 32-bit words."""
        cap_fp, cap_pk = region_caps(cs)
        assert len(out_key) == len(in_key) == 2 * W * cap_fp and len(out_pk) == len(in_pk) == W * cap_pk
        self._words(3, W, me, cs)
        self._image(out_key, np.uint64)
        self._image(in_key, np.uint64)
        self._image(out_pk, np.uint32)
        self._image(in_pk, np.uint32)
        return self

    def probe_slab(self, packed, reply):
        self._words(4, int(packed), int(reply))
        return self

    def rehash(self, b2):
        self._words(5, b2)
        return self

    def route_headers(self, received, pk, zero, counters):
        self._words(6, int(received), int(pk), int(zero))
        self._image(counters, np.uint64)
        return self

    def new_list(self, dev, W, cap, cs, counters, reply):
        assert len(counters) == (W * ROUTE_SEGS if dev else MAX_SHARDS) and len(reply) == W * cap
        self._words(7, int(dev), W, cap, cs)
        self._image(counters, np.uint64)
        self._image(reply, np.uint8)
        return self

    def dump(self):
        self._words(8)
        return self

    def layout(self, entries):
        """entries: (b0, b, b2, hi, lo, slot index, word)."""
        self._words(9, len(entries))
        self._image([w for e in entries for w in e], np.uint64)
        return self

    def write(self, path):
        with open(path, "wb") as f:
            f.write(b"".join(self.parts))
        return path


def region_caps(cs):
    """(records of a 16-byte region, 32-bit words of a packed one) at sub-slab capacity cs."""
    return ROUTE_HDR + ROUTE_SEGS * cs, PK_WORDS * (PK_HDR + ROUTE_SEGS * cs)


def slab_gy(groups, per):
    """The engine's blocks per group of the slab kernels (BfsEngine::slab_gy), to size a case that
    needs several grid-stride rounds; the program computes its own."""
    return max(1, min((per + BLOCK - 1) // BLOCK, max(1, 2048 // max(1, groups))))


def hex_words(s):
    return [int(s[k:k + 16], 16) for k in range(0, len(s), 16)]


def run_cpu(bin_, scenario, tmp_path, name="scenario.bin"):
    """A run that makes no GPU call (layout): plain subprocess."""
    path = scenario.write(os.path.join(str(tmp_path), name))
    out = subprocess.run([bin_, path], check=True, capture_output=True, text=True, timeout=120)
    return json.loads(out.stdout)["results"]


class GpuRunner:
    """One fresh child process per run, under its own time limit. A run that ends by a signal, an
    abort, its time limit or any error of the program poisons the runner: every later run fails at
    once, without starting another GPU process."""

    def __init__(self, bin_):
        self.bin = bin_
        self.poisoned = None

    def run(self, scenario, tmp_path, limit=60, name="scenario.bin"):
        assert self.poisoned is None, f"an earlier run of tablecheck failed ({self.poisoned}): no further GPU run"
        path = scenario.write(os.path.join(str(tmp_path), name))
        out = subprocess.run(["timeout", "-k", "10", str(limit), self.bin, path], capture_output=True, text=True)
        if out.returncode != 0:
            self.poisoned = f"exit status {out.returncode}: {out.stderr.strip()[-400:]}"
            raise AssertionError(f"tablecheck failed, {self.poisoned}")
        return json.loads(out.stdout)["results"]
