"""Stage C alone (irdm_qpsk_demod_batch, irdm_qpsk_demod_packed_batch: demod_seq_kernel, demod_par_kernel, demod_export of
csrc/demod.hip) without a GPU: the designed frames of tests/stage_c_cases.py -- lengths on either side of every decision,
the end-of-frame rule, the unique word on either side of the hard and the soft check under every input direction, the
timing loop at its limits, exact zeros under the PLL, noise -- through the product on the HIP emulation
(tests/emul_build.py) with either decimator, each record compared with the oracle's orc_qpsk_demod bit for bit (both
sides use the host's libm here), then the batch reversed, the rows padded with 1e30, and the packed export; each decimator in
a process of its own.  stage_c_cases.coverage() is asserted there.  tests/test_gpu_stage_c.py runs the same on the card."""
import json
import os
import subprocess
import sys

import pytest

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))

# the symbol counts the packed export is checked at: the last word (441 .. 447), a word of one byte (12, 100), a last byte
# of 1, 2 and 3 symbols (13, 14, 15), symbol counts that are no multiple of 16
EXPORT_COUNTS = {1: (12, 13, 14, 15, 16, 17, 100, 101, 191, 192, 441, 444, 447), 0: (12, 13, 14, 15, 100, 191, 444)}


def run_case(gardner, timeout=900):
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "stage_c_emul_run.py"), str(gardner)], env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


@pytest.mark.parametrize("gardner", (1, 0))
def test_designed_frames_match_the_oracle(gardner):
    res = run_case(gardner)
    assert 120 <= res["cases"] <= 160 and res["accepted"] >= 0.7 * res["cases"], res
    assert res["coverage"]["ns_441"] and res["coverage"]["ns_447"] and res["coverage"]["soft_rejected"], res
    assert set(EXPORT_COUNTS[gardner]) <= set(res["packed_symbol_counts"]), res
