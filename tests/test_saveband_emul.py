"""Saving the band (csrc/frontend.hip requant_kernel, csrc/frontend.cpp irdm_frontend_save / irdm_requantize_device) without a
GPU: the product's sources on the HIP emulation (tests/frontend_emul_build.py, tests/resample_emul_build.py), driven by
tests/saveband_emul_run.py in a process of its own.  The recording equals the numpy restatement of the quantiser
(tests/saveband_model.py) applied to the front end's model output, byte for byte, statistics included."""
import json
import os
import subprocess
import sys

import pytest

import frontend_emul_build
import resample_emul_build
import saveband_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emul_lib():
    return frontend_emul_build.build()


def run_case(lib, case, timeout=1800):
    env = dict(os.environ, IRDM_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(HERE, "saveband_emul_run.py"), case], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_requantiser_equals_the_numpy_model(emul_lib):
    """irdm_requantize_device: ci8 and ci16, gains 1 / 0.37 / 64, n in {0, 1, 2, 3, 63, 64, 65, 255, 257, 2^16 + 7}, input and
    output each at sample offsets 0, 1, 3 of a larger buffer; ties, rails, overflow, NaN, +-Inf, denormals and +-0 among the
    values: bytes and statistics exactly the model's, nothing written outside the output"""
    res = run_case(emul_lib, "kernel")
    assert res["calls"] == 2 * len(sm.GAINS) * len(sm.KERNEL_SIZES) * len(sm.OFFSETS) ** 2


def test_saved_band_equals_the_model_through_the_stage_entries(emul_lib):
    """irdm_frontend_save behind irdm_frontend_run_device / _finish_device: D = 2 at 4 MS/s, ci8 and cf32 captures of
    2^18 + 12345 samples, q = 14418, pieces of 4099 samples, whole and in ragged feeds; ci8 / ci16 recordings = the numpy
    model on the front end model's output, cf32 = its bytes; statistics and sample count match"""
    res = run_case(emul_lib, "stage")
    assert res == {"ci8": 6, "cf32": 6}


def test_saved_band_equals_the_model_through_the_rational_object():
    """the same behind irdm_frontend_create_rational at 11.2 -> 10 MS/s (25 / 28), against tests/resample_model.py's output"""
    res = run_case(resample_emul_build.build(), "rational")
    assert res == {"25/28": 6}


def test_reset_refusals_stop_and_saving_off(emul_lib):
    """irdm_frontend_reset mid-stream, then a second stream: exactly its bytes and statistics; a sink that returns non-zero
    makes the call return -1; irdm_frontend_save after the first sample (and with a bad field) returns -1; with saving off
    (never on, or turned off with NULL) the outputs are the model's, as before"""
    res = run_case(emul_lib, "props")
    assert res["reset"][0] > 0 and res["stop"] == [2 * 4099, 2 * 4099]
