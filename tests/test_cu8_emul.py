"""IRDM_FMT_CU8 (rtl_sdr's unsigned 8-bit I/Q) without a GPU: the product's sources on the HIP emulation, driven by
tests/cu8_emul_run.py in a process of its own.  Each run equals the emulated cf32 context on (u - 127.5) / 128 bit for bit,
and the oracle on that stream; a cu8 capture through either front end gives the band of the converted cf32 capture."""
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


def run_case(lib, case, timeout=900):
    env = dict(os.environ, IRDM_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(HERE, "cu8_emul_run.py"), case], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_cu8_2mhz(emul_lib):
    """generic K1 and the any-M decimator: whole stream, four chunks at pipeline_depth 1, sequential scan.  (The oracle
    alone decodes 6 of 6 frames of this scene at scales 512 and 2048, no component at a rail.)"""
    res = run_case(emul_lib, "2mhz")
    assert set(res) == {"whole", "chunked_depth1", "sequential_scan"}
    for name, s in res.items():
        assert s["bursts"] >= 4 and s["demods"] >= 3 and s["records"] > 0, (name, s)


def test_cu8_12mhz_two_chunks(emul_lib):
    """K1 p32<14> and the register-resident decimator at M = 48, in two chunks"""
    s = run_case(emul_lib, "12mhz")["two_chunks_depth1"]
    assert s["bursts"] >= 2 and s["demods"] >= 2 and s["records"] > 0, s


def test_cu8_through_k0():
    """D = 5: the cu8 capture's band = the converted cf32 capture's, whole and in ragged feeds; 5 and 7 stay refused"""
    res = run_case(frontend_emul_build.build(), "k0")
    assert res["outputs"] > 0 and res.get("refused_5") and res.get("refused_7"), res


def test_cu8_through_k0r():
    """2.4 -> 2.5 MS/s (25/24): likewise"""
    res = run_case(resample_emul_build.build(), "k0r")
    assert res["outputs"] > 0 and res.get("refused_5") and res.get("refused_7"), res
