"""Receiver I/Q imbalance without a GPU: the kernels of csrc/iq_moments.hpp and csrc/iq_balance.hpp on the HIP emulation
against the numpy model of tests/balance_model.py, irdm_iq_balance and option iq_moments through irdm_feed_host on a scene
with 1 dB and 5 degrees of imbalance planted; each case in a process of its own.  And the oracle alone: what the feature
rests on."""
import json
import os
import subprocess
import sys

import pytest

import balance_checks as bc
import emul_build
import irdm

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(*case, timeout=1500):
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "balance_emul_run.py")] + [str(c) for c in case], env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_balance_kernel_equals_the_model():
    """all eight formats, n in 0 .. 5, 255 .. 257, 4095 .. 4097 and 65536 + 3, src 0 .. 3 samples and dst 0 and 1 sample behind
    a 16-byte boundary, three coefficient pairs with the identity among them, cf32 with NaN, Inf, -0.0 and subnormals and in
    place: every bit the model's, the guard bytes untouched"""
    res = run_case("balance")
    assert res["cases"] == 8 * 13 * 4 * 2 and res["in_place"] == 13 * 4 * 2, res


def test_balance_refusals():
    """an unknown format, misaligned pointers, overlapping buffers, coefficients out of range: -1, nothing written"""
    assert run_case("refusals")["formats"] == 8


def test_moments_kernel_equals_the_model():
    """the same sizes, alignments and formats: counts exact, sums within N 2^-52 sum|term| of the float64 model's, gain and
    phase within 1e-6 from 4096 samples on; non-finite samples left out and counted wherever they lie; two launches give
    identical bytes; valid = 0 where there is nothing to judge"""
    res = run_case("moments")
    assert res["cases"] == 8 * 13 * 4 and res["left_out"] > 100, res


def test_oracle_facts():
    """CPU only: the clean scene gives 12 frames and no image; with 1 dB and 5 degrees planted it gives 24 frames with ok, of
    which the rule counts at least 8 as images; the model-corrected stream gives 12 frames, no image, and the clean scene's
    payload bits"""
    out = bc.oracle_facts()
    print(out)
    assert out["y"]["frames"] == 24


@pytest.mark.parametrize("depth", (0, 3))
def test_pipeline_with_balance_equals_the_corrected_stream(depth):
    """a context with irdm_iq_balance fed the impaired stream in chunks of 262 144 samples through the staging buffer
    (depth 0) and the ring slot (depth 3) yields the records of a plain context fed the model-corrected stream, bit for bit,
    and agrees with the oracle on that stream; option iq_moments reads below -60 dB on it; irdm_reset clears the moments
    and keeps the balance; a change in mid-stream and a device feed are refused"""
    res = run_case("pipeline", depth)
    assert res["demods"] == 12 and res["frames"] == 12, res


@pytest.mark.parametrize("fmt", (irdm.FMT_CI8, irdm.FMT_CI16))
@pytest.mark.parametrize("depth", (0, 3))
def test_pipeline_with_balance_from_integer_wire_formats(depth, fmt):
    """the same with the ci8 (scale 256) and ci16 renderings of the impaired stream as wire format, against a plain cf32
    context fed the model's correction of their conversion"""
    assert run_case("wire", depth, fmt)["demods"] >= 10


@pytest.mark.parametrize("depth", (0, 3))
def test_stream_moments_find_the_planted_imbalance(depth):
    """option iq_moments on the impaired stream: the model's figures, within 0.01 dB and 0.05 degrees of the planted 1 dB and
    5 degrees; -1 without the option, for a member of a group, and irdm_iq_balance on a context that is not cf32"""
    res = run_case("stream_moments", depth)
    assert res["demods"] == 24 and abs(res["gain_db"] - 1.0) <= 0.01, res
