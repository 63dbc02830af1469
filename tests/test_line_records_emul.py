"""The records of the two frame line estimators (irdm_symbol_clock_batch, irdm_fine_freq_batch) without a GPU: the kernels
of csrc/symbol_clock.hpp and csrc/fine_freq.hpp on the HIP emulation give, for every frame of tests/line_records.py, the
bytes of tests/golden/line_records.json -- the bytes the MI355X gives (tests/test_gpu_line_records.py)."""
import json
import os
import subprocess
import sys

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


def test_records_are_the_pinned_bytes():
    """the kernel frames of clock_checks and fine_freq_checks (lengths 63 / 64 / 65 / 255 / 1910 / 4439 / 4440; zero, NaN, Inf,
    noise; the line on either edge of the grid and beyond it) and their batches of 65 over launches of 64: 87 + 95 records"""
    env = dict(os.environ, IRDM_LIB=emul_build.build())
    p = subprocess.run([sys.executable, os.path.join(HERE, "line_records_emul_run.py")], env=env, capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(res)
    assert res["compared"] == 87 + 95
