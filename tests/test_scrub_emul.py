"""Option scrub without a GPU: the kernel of csrc/scrub.hpp on the HIP emulation, exact against the numpy model of
tests/scrub_model.py through irdm_scrub_device, and options scrub / scrub_limit_log2 through irdm_feed_host on a scene with
NaN, Inf and 1e30 written into the gaps between its bursts; each case in a process of its own.  And the oracle alone: what
the option is for."""
import json
import os
import subprocess
import sys

import pytest

import emul_build
import scrub_checks as sc

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(*case, timeout=1500):
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "scrub_emul_run.py")] + [str(c) for c in case], env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_kernel_equals_the_model():
    """n in 0 .. 5, 255 .. 257, 4095 .. 4097 and 65536 + 3, the buffer 0 and 1 sample behind a 16-byte boundary; no bad
    sample, all bad, about 1 %, and single ones at the head, the tail, the edge of a wavefront and of a workgroup, in I, in Q
    and in both; quiet and signalling NaN, +-Inf and the float behind +-2^e zeroed, +-2^e, -0.0 and subnormals kept, at
    e = 0, 24, 40, 127: the buffer and the guard bytes exact, all six figures exact, a second pass changes and counts
    nothing"""
    assert run_case("kernel")["cases"] > 500


def test_other_formats_and_refusals():
    """the seven formats that are not cf32: 0, the buffer untouched; -1 for an unknown format, a pointer that is not aligned
    to a sample and a limit outside 0 .. 127"""
    assert run_case("refusals")["formats"] == 7


def test_oracle_recovers_on_the_scrubbed_stream():
    """CPU only: the oracle on the model-scrubbed stream gives the clean scene's 12 frames, every unique word ok"""
    assert len(sc.oracle_clean().demods) == 12


def test_oracle_alone_is_blind_behind_a_bad_sample():
    """CPU only: the oracle on the stream as recorded (a NaN at sample 0) finds nothing at all"""
    assert sc.oracle_blind_case() == dict(bursts=0, demods=0)


@pytest.mark.parametrize("depth", (0, 3))
def test_pipeline_with_scrub_equals_the_scrubbed_stream(depth):
    """a context with scrub on, fed the stream as recorded in chunks of 262 144 samples through the staging buffer
    (depth 0) and the ring slot (depth 3), yields the records of a context without it fed the model-scrubbed stream, bit for
    bit, and agrees with the oracle on that stream; irdm_scrub_stats equals the model's figures in stream coordinates;
    irdm_reset clears them; a change of either option in mid-stream and a device feed with the option on return -1"""
    res = run_case("pipeline", depth)
    assert res["demods"] == 12 and res["frames"] == 12, res
