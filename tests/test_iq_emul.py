"""Exchanged I and Q without a GPU: the exchange kernel of csrc/iq_swap.hpp and the sense kernel of csrc/bitlayer.hip on the
HIP emulation -- the exchange exact against numpy for all eight formats, irdm_iq_sense_batch against the model of
tests/iq_sense_model.py field for field, and options iq_sense / swap_iq through irdm_feed_host on a scene of IRA, IBC and
IDA frames fed as it is and with its components exchanged; each case in a process of its own."""
import json
import os
import subprocess
import sys

import pytest

import emul_build
import irdm

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(*case, timeout=1500):
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "iq_emul_run.py")] + [str(c) for c in case], env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_exchange_kernel_equals_numpy():
    """all eight formats, n in 0 .. 4097, the buffer 0 .. 3 samples behind a 16-byte boundary: exact, the guard bytes
    untouched, the identity applied twice, -1 for an unknown format and a pointer that is not sample-aligned"""
    assert run_case("swap")["cases"] == 8 * 11 * 4


def test_votes_equal_the_model():
    """irdm_iq_sense_batch on frame_corpus and ida_corpus of two seeds, as they are and exchanged, the cases without LLRs
    and the cut frames among them; the model alone first: at least 20 recorded votes of each kind, none in the wrong sense"""
    res = run_case("votes")
    assert min(res["kinds"]) >= 20 and res["odd"] > 0 and res["no_llr"] > 0, res


@pytest.mark.parametrize("depth", (0, 3))
def test_pipeline_votes_and_swap_iq(depth):
    """the scene (a) as it is: 12 recorded votes; (b) exchanged: 12 exchanged votes, every frequency mirrored; (c) exchanged
    with swap_iq: (a)'s records bit for bit; in chunks of 262 144 samples through the staging buffer (depth 0) and the
    ring slot (depth 3); a change of swap_iq in mid-stream and a device feed with it on return -1; irdm_reset clears"""
    assert run_case("pipeline", depth, irdm.FMT_CF32)["frames"] == 12


@pytest.mark.parametrize("depth,fmt", ((0, irdm.FMT_CI8), (3, irdm.FMT_CI8), (0, irdm.FMT_CI16), (3, irdm.FMT_CI16)))
def test_swap_iq_in_ci8_and_ci16(depth, fmt):
    """(c) on siggen.to_ci8 / to_ci16 of the scene and of its exchange"""
    assert run_case("pipeline", depth, fmt)["frames"] == 12


def test_random_payloads_do_not_vote():
    """(d) siggen.standard_scene: frames, no votes, verdict 0"""
    assert run_case("random", 3)["frames"] >= 5
