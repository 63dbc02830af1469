"""TEST INFRASTRUCTURE: the symbol timing estimator (csrc/fine_time.hpp) on the CPU emulation against
tests/fine_time_model.py.  Started by tests/test_fine_time_emul.py in a process of its own with IRDM_LIB pointing at an
emulated build.
Usage: python fine_time_emul_run.py <case> [write-golden]
write-golden (case stage): tests/golden/fine_time_records.json is written from this run before it is compared."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import fine_time_checks as fc       # noqa: E402
import irdm                         # noqa: E402


def stage(write_golden=False):
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64, pipeline_depth=0)
    try:
        return fc.stage_cases(p, write_golden)      # (batches of 65 frames: two calls' worth of max_bursts_per_chunk 64)
    finally:
        p.close()


def context():
    """the 2 MHz seed-3 scene through contexts with the option off and on, both record paths, one feed and three, reset,
    the bit layer's records; a group refuses the option"""
    seen = fc.context_checks((2_000_000, 3, 0.05), 14)
    fc.group_refuses()
    return seen


def main():
    case = sys.argv[1]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    res = stage("write-golden" in sys.argv[2:]) if case == "stage" else context()
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
