"""irdm_prime_host without a GPU: the product's host path on the HIP emulation, primed from the recording's own head, against
the CPU oracle run over P || x (P: the 512-frame prefix tiled from the head, built in numpy by tests/prime_checks.py) with
start time T0'; each case in a process of its own.  2 MHz cf32."""
import json
import os
import subprocess
import sys

import pytest

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(*case, timeout=1500):
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "prime_emul_run.py")] + [str(c) for c in case], env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


@pytest.mark.parametrize("depth", (0, 3))
def test_full_scene_finds_the_six_early_bursts(depth):
    """standard_scene(2 MHz, 3 000 000 samples, 16 bursts, seed 3, first_start=40 000): the primed context's records equal
    the oracle's over P || x in every compared field, 16 bursts and 16 frames; irdm_prime_host after a feed returns -1 and
    changes nothing; after irdm_reset the same context gives the plain run's records, 10 bursts and 10 frames"""
    res = run_case("scene", "full", depth)
    assert res["primed"] == dict(bursts=16, demods=16) and res["plain"] == dict(bursts=10, demods=10, compared=True), res


@pytest.mark.parametrize("depth", (0, 3))
def test_recording_shorter_than_the_priming_length(depth):
    """a 700 000-sample excerpt (341 frames) primed from itself, tiled: 6 bursts and 6 frames, equal to the oracle's over
    P || x, where the plain run finds nothing at all"""
    res = run_case("scene", "excerpt", depth)
    assert res["primed"] == dict(bursts=6, demods=6) and res["plain"] == dict(bursts=0, demods=0, compared=False), res


@pytest.mark.parametrize("depth", (0, 3))
def test_swap_balance_and_scrub_apply_to_the_prefix(depth):
    """swap_iq, irdm_iq_balance and scrub on together: byte for byte the records of a plain context with the three on, start
    time T0', fed P || x; the scrub's figures count the recording alone"""
    assert run_case("options", depth) == dict(demods=6)


@pytest.mark.parametrize("depth", (0, 3))
def test_side_passes_describe_the_recording_alone(depth):
    """input_stats, iq_moments, scrub and spectrum_frames: exactly the results of a plain context fed x alone with start time
    T0, positions and row times included"""
    assert run_case("side", depth) == dict(rows=4)
