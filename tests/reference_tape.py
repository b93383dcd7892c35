"""What the REAL reference computed, for tests that compare the oracle with it.

Where oracle/_ref was built (__graft_entry__.build() with the reference checkout present) the reference runs live,
as before, and every value it produced must also equal the one stored under tests/golden/reference/ (a drift of the
checkout, the stand-ins or the recipe fails instead of passing unnoticed).  Everywhere else the stored values stand in
for it, so that the comparison runs from the repository alone.  Observations the tests compare bit for bit are stored
as a SHA-256 digest when they are large (whole map buffers), as they are otherwise; values a test computes with are
stored as they are.  tests/golden/make_reference_golden.py rewrites the files (FUELMI_RECORD_REFERENCE=1)."""
import hashlib
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
RAW_MAX = 4096  # bytes of a canonical observation up to which it is stored as it is


def _canon(a):
    # one form per value: np.array_equal compares values, not dtypes, and -0.0 == 0.0
    return np.array(a, dtype=np.float64, order="C") + 0.0


def digest(a):
    a = _canon(a)
    h = hashlib.sha256(repr(a.shape).encode())
    h.update(a.tobytes())
    return h.hexdigest()


class Tape:
    """The reference's observations of one test, in the order the test makes them."""

    def __init__(self, name, live, record=False):
        self.path = os.path.join(GOLDEN, re.sub(r"[^A-Za-z0-9_.-]+", "_", name) + ".npz")
        self.live, self.record = live, live and record
        self.seq = 0
        self.out = {}
        self.stored = None
        if not self.record:
            assert os.path.exists(self.path), \
                "%s is missing (tests/golden/make_reference_golden.py writes it)" % os.path.relpath(self.path)
            with np.load(self.path) as z:
                self.stored = {k: z[k] for k in z.files}

    def _next(self):
        self.seq += 1
        return "%04d" % (self.seq - 1)

    def _keep(self, key, kind, v):
        if self.record:
            self.out[key + kind] = v
        else:
            assert key + kind in self.stored, "%s: no stored observation %s%s" % (self.path, key, kind)
            s = self.stored[key + kind]
            assert s.shape == np.shape(v) and np.array_equal(s, v), \
                "the reference's observation %s differs from %s" % (key, os.path.relpath(self.path))

    def equal(self, ours, theirs=None):
        """assert np.array_equal(ours, <the reference's value>); theirs: a callable, used only when live"""
        key = self._next()
        if self.live:
            t = np.asarray(theirs())
            assert np.array_equal(ours, t), key
            c = _canon(t)
            self._keep(key, "_raw" if c.nbytes <= RAW_MAX else "_sha", c if c.nbytes <= RAW_MAX else np.array(digest(c)))
            return
        if key + "_raw" in self.stored:
            assert np.array_equal(ours, self.stored[key + "_raw"]), key
        else:
            assert digest(ours) == str(self.stored[key + "_sha"]), key

    def value(self, theirs):
        """the reference's value itself (live: computed; else the stored one), for a test that computes with it"""
        key = self._next()
        if self.live:
            v = np.asarray(theirs())
            self._keep(key, "_val", v)
            return v
        return self.stored[key + "_val"]

    def close(self):
        if self.record:
            os.makedirs(GOLDEN, exist_ok=True)
            np.savez_compressed(self.path, **self.out)
        elif self.stored is not None:
            assert self.seq == len(self.stored), "%s holds %d observations, the test made %d" % (
                os.path.relpath(self.path), len(self.stored), self.seq)
