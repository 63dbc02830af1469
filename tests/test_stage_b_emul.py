"""Stage B alone (irdm_downmix_burst: the rotator checkpoints, the three decimators, post_tiles / post_cfo, rot_phase_rows,
post2 of csrc/downmix.hip and csrc/fir_reg.hip) without a GPU: the designed burst windows of tests/stage_b_cases.py -- every
early return of burst_downmix.c, frames shorter than the CFO estimator's input and longer than the demodulator takes,
the simplex rules -- through the product on the HIP emulation (tests/emul_build.py) at every class of stream position,
each call compared with the oracle's orc_downmix_process the way parity.compare compares a frame; each case in a process of
its own.  tests/test_gpu_stage_b.py runs the same on the card."""
import json
import os
import subprocess
import sys

import pytest

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))

RATES = (725_000, 2_000_000, 2_500_000, 4_000_000, 10_000_000, 12_000_000, 20_000_000)


def run_case(fs, order, *options, timeout=900):
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "stage_b_emul_run.py"), str(fs), str(order)] + list(options), env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


@pytest.mark.parametrize("fir_order", (1, 0))
@pytest.mark.parametrize("fs", RATES)
def test_designed_windows_match_the_oracle(fs, fir_order):
    """the whole corpus at every start class (the two whose window ends where the detector's feed block had not delivered it
    are the regression test of irdm_downmix_burst using its caller's whole window), then stage_b_cases.coverage: all six
    drop reasons, both sides of reason 4, both directions, frames of 1910 and 4440 samples, the short and the long CFO input"""
    res = run_case(fs, fir_order)
    assert res["calls"] >= 36 * 6 and all(res["hist"][str(r)] >= 1 for r in range(6)), res


@pytest.mark.parametrize("option", ("post_generic", "fir_generic"))
@pytest.mark.parametrize("fs", (2_000_000, 10_000_000))
def test_designed_windows_generic_kernel_forms(fs, option):
    """test hooks post_generic (the runtime-tap-count instances of post_tiles / post_cfo / post2) and fir_generic (always the
    any-M decimator): same frames"""
    res = run_case(fs, 1, option + "=1")
    assert res["calls"] >= 36 * 6, res
