"""A receiver's DC offset without a GPU: the kernels of csrc/dc_block.hpp on the HIP emulation against the numpy model of
tests/dc_model.py, irdm_dc_block through irdm_feed_host on a stream with a DC of 0.03 (1 + 0.6j) planted; each case in a
process of its own.  And the oracle alone: what the feature is for."""
import json
import os
import subprocess
import sys

import pytest

import dc_checks as dc
import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(*case, timeout=1500):
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "dc_emul_run.py")] + [str(c) for c in case], env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_dc_kernels_equal_the_model():
    """all eight formats, n in 0 .. 5, 255 .. 257, 4095 .. 4097 and 65536 + 3, src and dst 0 and 1 sample behind a 16-byte
    boundary, blocks of 4096 with an edge at sample 1, inside a 16-byte piece, at a wavefront's and at a workgroup's edge, a
    seed and the sums of a block under way; cf32 with quiet and signalling NaN, +-Inf, +-1e30, +-64 and the floats beside
    them, -0.0 and subnormals: output bytes, guard bytes and state_io exact; a second call gives the same bytes; the 8-byte
    formats in place"""
    res = run_case("kernel")
    assert res["cases"] == 8 * 13 * 4 and res["again"] == 8 * 4 * 4 and res["in_place"] == 3 * 13 * 4, res


def test_dc_refusals_and_host_mean():
    """an unknown format, a block length outside 12 .. 24, misaligned pointers, overlapping buffers, a mean that is not finite
    or beyond +-64: -1, nothing written; irdm_dc_mean_host equals the model for every format"""
    assert run_case("refusals")["formats"] == 8


def test_dc_carry():
    """one stream cut into calls of 1, 4095, 4097 and 100 003 samples gives the bytes and the final state of a single call"""
    assert run_case("carry")["streams"] == 4


def test_what_it_is_for():
    """CPU only, the oracle alone.  The clean stream gives 13 frames, all ok.  With a DC of 0.03 (1 + 0.6j) -- 4.4 dB under the
    bursts' amplitude -- the detector still finds 13 bursts and 3 frames are left, the three off the centre channel.  The
    model-corrected stream (blocks of 2^16, seeded from its own head as the binary seeds a recording) gives back every one
    of the clean run's frames, ok, with the clean run's timestamps and bits."""
    out = dc.oracle_facts()
    print(out)
    assert out["clean"] == out["clean_ok"] == 13, out
    assert out["dc"] < out["clean"] and out["dc"] == 3 and out["dc_same"] == 3, out
    assert out["fixed"] == out["fixed_ok"] == 13 and out["fixed_bits"] == 13 and out["fixed_same"] == 13, out


@pytest.mark.parametrize("depth", (0, 3))
def test_pipeline_with_dc_block_equals_the_corrected_stream(depth):
    """a context with irdm_dc_block (blocks of 2^16) fed the impaired stream in chunks of 262 144 and again of 98 304 samples,
    through the staging buffer (depth 0) and the ring slot (depth 3), yields the records of a plain context fed
    dc_model(stream), bit for bit and alike for both chunkings, and agrees with the oracle on that stream; irdm_dc_stats
    equals the model's figures; irdm_reset clears the stream state and keeps the setting; the refusals"""
    res = run_case("pipeline", depth)
    assert res["demods"] >= 12, res


@pytest.mark.parametrize("depth", (0, 3))
def test_pipeline_with_dc_block_from_ci16_full(depth):
    """the ci16-full rendering of the impaired stream as wire format, against a plain cf32 context fed the model's correction
    of its conversion"""
    assert run_case("wire", depth)["demods"] >= 12


def test_composition_with_swap_and_balance():
    """swap_iq, irdm_dc_block and irdm_iq_balance on one context: the records of balance(dc_model(swap(x)))"""
    assert run_case("composition", 3)["bursts"] >= 12
