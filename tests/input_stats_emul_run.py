"""TEST INFRASTRUCTURE: the input statistics (csrc/input_stats.hpp) on the CPU emulation against tests/inputstats_model.py.
Started by tests/test_input_stats_emul.py in a process of its own with IRDM_LIB pointing at an emulated build.
Usage: python input_stats_emul_run.py <case>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import input_stats_checks as ic     # noqa: E402
import irdm                         # noqa: E402


def main():
    case = sys.argv[1]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    if case == "stage":
        res = ic.stage_cases()
    elif case == "context":
        res = ic.context_cuts()
    elif case == "frontend":
        res = ic.frontend_cuts()
    else:
        raise SystemExit("unknown case")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
