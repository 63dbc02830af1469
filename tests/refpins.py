"""The reference's outputs for the tests that pin the oracle to the reference's own code (oracle/_ref), held as data.

Where oracle/_ref is built, a test computes the reference's output live and asserts the oracle's is the same, bit for bit;
the SHA-256 of the reference's output must also equal the one recorded under the same name in tests/golden/ref_digests.json
(IRDM_WRITE_GOLDEN=1 records it instead).  Where oracle/_ref is not built, the oracle's output is checked against the
recorded digest: the same bit-for-bit assertion against the same reference output.  Test modules use the fixture with
`from refpins import refpins`."""
import hashlib
import json
import os

import numpy as np
import pytest

import orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_digests.json")


def as_bytes(x):
    """bytes of an output: arrays with their dtype and shape, numbers exactly, strings as UTF-8, lists and tuples in order"""
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    if isinstance(x, str):
        return x.encode()
    if isinstance(x, np.ndarray):
        return ("%s%r" % (x.dtype.str, x.shape)).encode() + np.ascontiguousarray(x).tobytes()
    if isinstance(x, np.generic):
        return x.dtype.str.encode() + x.tobytes()
    if isinstance(x, (bool, int)):
        return b"i%d;" % int(x)
    if isinstance(x, float):
        return b"d" + np.float64(x).tobytes()
    if isinstance(x, (list, tuple)):
        return b"(" + b",".join(as_bytes(p) for p in x) + b")"
    raise TypeError("no byte form for %r" % type(x))


class Pins:
    def __init__(self, lib):
        self.lib = lib                                       # oracle/_ref, or None
        self.want = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        self.write = lib is not None and os.environ.get("IRDM_WRITE_GOLDEN") == "1"
        self.recorded = {}

    def same(self, key, ours, ref=None):
        """ours: the oracle's output; ref: the reference's output for the same input (given whenever self.lib is)"""
        ours = as_bytes(ours)
        if self.lib is not None:
            ref = as_bytes(ref)
            assert ours == ref, key
        digest = hashlib.sha256(ref if self.lib is not None else ours).hexdigest()
        if self.write:
            self.recorded[key] = digest
            return
        assert key in self.want, "%s: no recorded reference output (IRDM_WRITE_GOLDEN=1 where oracle/_ref is built)" % key
        assert digest == self.want[key], "%s differs from the reference's recorded output" % key


@pytest.fixture(scope="session")
def refpins():
    p = Pins(orc.ref())
    yield p
    if p.write:                  # (each test module has its own instance: merge into what is on disk)
        want = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        want.update(p.recorded)
        with open(GOLDEN, "w") as f:
            json.dump(want, f, indent=1, sort_keys=True)
            f.write("\n")
