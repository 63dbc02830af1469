"""TEST INFRASTRUCTURE: the per-burst resampler (csrc/burst_resample.hpp, option "burst_resample") on the CPU emulation
against tests/burst_resample_model.py and the oracle.  Started by tests/test_burst_resample_emul.py and
tests/test_burst_resample_host.py in a process of its own with IRDM_LIB pointing at an emulated build.
Usage: python burst_resample_emul_run.py <case> [args]"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import burst_resample_checks as bc      # noqa: E402
import burst_resample_model as bm       # noqa: E402
import irdm                             # noqa: E402


def main():
    case = sys.argv[1]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    res = bc.CASES[case](*[int(a) for a in sys.argv[2:]])
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
