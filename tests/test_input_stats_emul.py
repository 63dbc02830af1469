"""The input statistics (option input_stats, irdm_input_stats_device, the front end's getter) without a GPU: the kernel of
csrc/input_stats.hpp on the HIP emulation against the integer / fsum model of tests/inputstats_model.py, each case in a
process of its own."""
import json
import os
import subprocess
import sys

import frontend_emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(case, timeout=900):
    env = dict(os.environ, IRDM_LIB=frontend_emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "input_stats_emul_run.py"), case], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_stage_level_equals_the_model():
    """every format, n in {0, 1, 3, 63, 64, 65, 255, 4101, 2^20 + 7}, bases 0 / 1 / 3 samples past a 16-byte boundary, rails
    at the first and last sample, all-rail buffers (int16: the sum of squares 2^50), cf32 with NaN, Inf, +-1.0, subnormals"""
    assert run_case("stage")["cases"] >= 6 * 9 * 3 + 6 + 10


def test_context_option_does_not_depend_on_the_cut():
    """whole, four chunks at pipeline_depth 1, ragged pieces: byte-identical structs equal to the model's"""
    res = run_case("context")
    assert res["n_samples"] > 2_000_000


def test_frontend_getter_covers_the_capture():
    res = run_case("frontend")
    assert res["n_samples"] == 5 * 4096 + 777
