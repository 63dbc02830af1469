"""The symbol clock estimator (option symbol_clock, irdm_symbol_clock_batch) without a GPU: the kernel of
csrc/symbol_clock.hpp on the HIP emulation against the float64 model of tests/clock_model.py, each case in a process of
its own.

Measured here, over the kernel-test frames of tests/clock_checks.py (the oracle's frames of the 10.025 MHz scene, lengths
63 / 64 / 65 / 1910 / 4440, batches of 1 / 63 / 65, zero / NaN / Inf / noise frames, two resampled frames): the largest
|eps_device - eps_model| is EPS_MEASURED of clock_checks.py; 4 x that is asserted, far under the 0.01 % the estimator may
take.  Flags and n are equal."""
import json
import os
import subprocess
import sys

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(case, timeout=900):
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "clock_emul_run.py"), case], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_kernel_equals_the_model():
    import clock_checks as cc
    res = run_case("stage")
    assert res["frames"] >= 5 + 9 + 6
    assert res["worst"] <= cc.EPS_TOL


def test_context_records_do_not_depend_on_depth_or_feeds():
    res = run_case("context")
    assert res["used"] >= 4
