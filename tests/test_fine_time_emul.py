"""The symbol timing estimator (option fine_time, irdm_fine_time_batch) without a GPU: the kernel of csrc/fine_time.hpp on the
HIP emulation against the float64 model of tests/fine_time_model.py, each case in a process of its own.

Measured here, over the kernel-test frames of tests/fine_time_checks.py (the oracle's 16 frames of the 2 MHz seed-3 scene,
cuts of them to 63 / 64 / 65 / 799 / 800 / 801 / 1309 / 1310 / 1311 / 4440 samples with the simplex flag both ways, batches of
1 / 63 / 65, zero / NaN / Inf / noise frames, synthetic frames with tau at -4.9, 0 and +4.9): the largest
|tau_device - tau_model| is 6.1e-14 samples against the 1e-9 asserted, and the largest relative difference of the qualities
5.2e-8 against 1e-6.  Flags and n are equal, and the kernel's sums are bit for bit those of
tests/golden/fine_time_records.json.  (With the sines and cosines of sinf's polynomials, which the other two line estimators
use, the first figure was 1.2e-8: csrc/frame_line.hpp, sc_sincos_turns_exact.)

Context, 2 MHz seed-3 scene: 16 frames applied, refined time - truth mean -32 ns, largest 256 ns (520 asserted, the model
test's bound), where the unrefined timestamp deviates from its own mean offset by up to 7.4 us."""
import json
import os
import subprocess
import sys

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(case, timeout=900):
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "fine_time_emul_run.py"), case], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    print(p.stdout)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_kernel_equals_the_model():
    import fine_time_checks as fc
    res = run_case("stage")
    print(res)
    assert res["frames"] == res["golden"] >= 16 + 2 * len(fc.CUTS) + 5 + 3
    assert res["worst"] <= fc.TAU_TOL and res["worst_quality"] <= fc.QUALITY_RTOL


def test_context_records_with_the_option_off_and_on():
    """the 2 MHz seed-3 scene: every field but timestamp bit for bit, every applied time within the model test's bound of
    truth where the unrefined timestamp wanders by more than 5 us, both record paths, one feed and three, irdm_reset, the
    polled records pair with the demodulator's, the bit layer's records, a group's refusal"""
    import fine_time_checks as fc
    res = run_case("context")
    print(res)
    assert res["full"] == res["packed"] >= 14 and res["reset"]
    assert res["worst_ns"] <= fc.TRUTH_TOL_NS[2_000_000] and res["unrefined_spread_ns"] > 5000.0
