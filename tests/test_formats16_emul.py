"""The full-precision int16 formats (IRDM_FMT_CI16_FULL, IRDM_FMT_SC16Q11) without a GPU: the product's sources on the HIP
emulation (tests/emul_build.py), driven by tests/formats16_emul_run.py in a process of its own.  Each run equals the
emulated cf32 context on v.astype(np.float32) * scale bit for bit, and the oracle on that stream."""
import json
import os
import subprocess
import sys

import pytest

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emul_lib():
    return emul_build.build()


def run_case(lib, case, timeout=900):
    env = dict(os.environ, IRDM_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(HERE, "formats16_emul_run.py"), case], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_formats16_2mhz(emul_lib):
    """generic K1 and the any-M decimator, both formats: whole stream, four chunks at pipeline_depth 1, sequential scan"""
    res = run_case(emul_lib, "2mhz")
    assert set(res) == {"%s_%s" % (f, c) for f in ("ci16-full", "sc16q11")
                        for c in ("whole", "chunked_depth1", "sequential_scan")}
    for name, s in res.items():
        assert s["bursts"] >= 4 and s["demods"] >= 3, (name, s)


def test_formats16_12mhz_two_chunks(emul_lib):
    """K1 p32<14> and the register-resident decimator at M = 48, in two chunks"""
    res = run_case(emul_lib, "12mhz")
    s = res["sc16q11_two_chunks_depth1"]
    assert s["bursts"] >= 2 and s["demods"] >= 2, s
