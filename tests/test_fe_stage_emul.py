"""The front end's shared load stage (csrc/fe_stage.hpp) without a GPU: the product's sources on the HIP emulation
(tests/resample_wide_emul_build.py), driven by tests/fe_stage_emul_run.py in a process of its own.  The assertions are those
of tests/fe_stage_cases.py, which tests/test_gpu_fe_stage.py makes on the GPU: every instantiation of K0, K0r and K0w that
differs in the load stage equals the plain C models bit for bit in all eight device formats, fed whole, in ragged feeds and
after a reset."""
import json
import os
import subprocess
import sys

import pytest

import fe_stage_cases as fc
import resample_wide_emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emul_lib():
    return resample_wide_emul_build.build()


@pytest.mark.parametrize("row", sorted(fc.ROWS))
def test_load_stage_equals_the_models_in_every_format(emul_lib, row):
    """eight formats x q = 14418, -32768; four tiles and an odd remainder, so a first tile in front of the stream, tiles
    wholly inside the chunk and a partial last one"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "fe_stage_emul_run.py"), row], env=dict(os.environ, IRDM_LIB=emul_lib),
                       capture_output=True, text=True, timeout=3600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert len(res) == len(fc.FORMATS) * len(fc.Q_LIST) and all(v > 0 for v in res.values()), res
