"""IRDM_FMT_CI32 (int32, v / 2^31) and IRDM_FMT_CI32_24 (24-bit samples in int32, v / 2^23) without a GPU: the product's
sources on the HIP emulation, driven by tests/ci32_emul_run.py in a process of its own.  Each run equals the emulated cf32
context on v.astype(float32) * scale bit for bit, and the oracle on that stream; a capture through either front end gives
the band of the converted cf32 capture; the input statistics equal an integer model."""
import json
import os
import subprocess
import sys

import pytest

import emul_build
import frontend_emul_build
import resample_emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emul_lib():
    return emul_build.build()


def run_case(lib, case, timeout=1500):
    env = dict(os.environ, IRDM_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(HERE, "ci32_emul_run.py"), case], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_ci32_2mhz(emul_lib):
    """generic K1 and the any-M decimator.  Format 8: a scene at scale 2^34 -- most values need more than 24 bits, so (float)v
    rounds -- with INT32_MIN and INT32_MAX among its samples (INT32_MAX converts to exactly 1.0), whole, in four chunks at
    pipeline_depth 1 and with the sequential scan.  Format 9: 24-bit values, whole and in four chunks.  The oracle alone gives
    at least 4 bursts and 3 demodulated frames on each.  5, 7 and 10 are refused."""
    res = run_case(emul_lib, "2mhz")
    runs = {"whole", "chunked_depth1", "sequential_scan", "whole_24", "chunked_depth1_24"}
    assert runs <= set(res)
    assert res["frac_over_24_bits"] > 0.5
    for name in runs:
        s = res[name]
        assert s["bursts"] >= 4 and s["demods"] >= 3 and s["records"] > 0, (name, s)
    assert res.get("refused_5") and res.get("refused_7") and res.get("refused_10"), res


def test_ci32_12mhz_two_chunks(emul_lib):
    """K1 p32<14> and the register-resident decimator at M = 48, in two chunks, both formats"""
    res = run_case(emul_lib, "12mhz")
    for key in ("two_chunks_depth1", "two_chunks_depth1_24"):
        s = res[key]
        assert s["bursts"] >= 4 and s["demods"] >= 3 and s["records"] > 0, (key, s)


def test_ci32_through_k0():
    """D = 5: the int32 capture's band = the converted cf32 capture's, whole and in ragged feeds, both formats, the extreme codes
    among the samples; 5, 7 and 10 stay refused"""
    res = run_case(frontend_emul_build.build(), "k0")
    assert res["outputs_8"] > 0 and res["outputs_9"] > 0, res
    assert res.get("refused_5") and res.get("refused_7") and res.get("refused_10"), res


def test_ci32_through_k0r():
    """2.4 -> 2.5 MS/s (25/24): likewise"""
    res = run_case(resample_emul_build.build(), "k0r")
    assert res["outputs_8"] > 0 and res["outputs_9"] > 0, res
    assert res.get("refused_5") and res.get("refused_7") and res.get("refused_10"), res


def test_ci32_input_stats():
    """the statistics kernel on the emulation against the model in Python integers: both formats, rails, extreme codes (the
    sum of squares past 64 bits), every size and two alignments; the context's option over one stream cut three ways gives
    one struct"""
    res = run_case(frontend_emul_build.build(), "stats")
    assert res["cases"] >= 2 * 10 * 2 + 2 + 6
    assert set(res["context"]) == {"ci32", "ci32-24"}
