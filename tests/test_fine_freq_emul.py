"""The carrier frequency estimator (option fine_freq, irdm_fine_freq_batch) without a GPU: the kernel of csrc/fine_freq.hpp
on the HIP emulation against the float64 model of tests/fine_freq_model.py, each case in a process of its own.

Measured here, over the kernel-test frames of tests/fine_freq_checks.py (the oracle's frames of the 10 MHz scene, lengths
63 / 64 / 65 / 255 / 1910 / 4439 / 4440, batches of 1 / 63 / 65, zero / NaN / Inf / noise frames, a frame with its line on
either edge of the grid and one 120 Hz beyond it): the largest |df_device - df_model| is 5.3e-6 Hz -- half an ulp of the
record's float at 65 Hz is 3.8e-6 -- against the 1e-3 Hz asserted, and the largest relative difference of the qualities
5.1e-8 against 1e-6.  Flags and n are equal."""
import json
import os
import subprocess
import sys

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(case, timeout=900):
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "fine_freq_emul_run.py"), case], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_kernel_equals_the_model():
    import fine_freq_checks as fc
    res = run_case("stage")
    print(res)
    assert res["frames"] >= 7 + 16 + 7
    assert res["worst"] <= fc.DF_TOL and res["worst_quality"] <= fc.QUALITY_RTOL


def test_context_records_with_the_option_off_and_on():
    """the 2 MHz seed-3 scene: every field but center_frequency bit for bit, applied frames within 4 Hz of truth where the
    PLL's value is 33 Hz off, both record paths, one feed and three, irdm_reset, the bit layer's records, a group's refusal"""
    import fine_freq_checks as fc
    res = run_case("context")
    print(res)
    assert res["full"] == res["packed"] >= 14 and res["reset"]
    assert res["worst"] <= fc.TRUTH_TOL and res["pll_worst"] > 15.0
