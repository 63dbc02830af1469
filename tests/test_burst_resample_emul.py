"""Option "burst_resample" without a GPU: burst_resample_kernel (csrc/burst_resample.hpp) and the chain around it on the HIP
emulation, each case in a process of its own (tests/burst_resample_emul_run.py, the checks of tests/burst_resample_checks.py).

Stage level, irdm_burst_resample_batch on rows of seeded noise plus a 30 kHz tone of 100, 101, 2047, 22 480, 65 536 and 3
samples and three impulse rows, one launch per ratio: res_len by the rule, the output the float32 model's bit for bit and
within 2e-6 of full scale of the float64 reference, the tone within 1 Hz, the impulses centred at i L / M.

Pipeline level, eight-burst scenes at 2.4, 2.05, 10.025 and 10.24 MS/s: with the option off the oracle's records (no frame whole
at 2.4 and 2.05 MS/s); with it on the same bursts, every frame that passed the unique word whole, its frequency within 50 Hz
and its time within 20 us of the scene's truth.  On the grid the option changes nothing and launches nothing.  Packed, parsed
and full records, pipeline_depth 0 and 3, several chunk sizes and a group of two emulated devices give the same records."""
import json
import os
import subprocess
import sys

import pytest

import burst_resample_checks as bc
import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(case, *args, timeout=900):
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "burst_resample_emul_run.py"), case] + [str(a) for a in args], env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


@pytest.mark.parametrize("L,M", bc.STAGE_RATIOS)
def test_kernel_equals_the_model(L, M):
    res = run_case("stage", L, M)
    assert res["rows"] == len(bc.STAGE_LENGTHS) + 3 and res["worst64"] <= 2e-6 and res["worst_hz"] <= 1.0


@pytest.mark.parametrize("fs", [2_400_000, 2_050_000, 10_025_000, 10_240_000])
def test_off_grid_frames_come_out_whole(fs):
    res = run_case("pipeline", fs)
    assert res["whole_on"] == res["frames"] >= 6 and res["worst_hz"] <= 50.0 and res["worst_us"] <= 20.0, res
    if fs in (2_400_000, 2_050_000):
        assert res["whole_off"] == 0


def test_on_the_grid_nothing_changes_and_nothing_is_launched():
    assert run_case("ongrid")["frames"] >= 6


def test_record_modes_depths_and_chunk_sizes_agree():
    assert run_case("modes")["frames"] >= 6


def test_group_of_two_takes_the_option():
    res = run_case("group")
    assert res["frames"] >= 6 and res["chunks"] == 2
