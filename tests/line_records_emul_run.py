"""TEST INFRASTRUCTURE: the records of the two frame line estimators (csrc/frame_line.hpp) on the CPU emulation against the
bytes of tests/golden/line_records.json.  Started by tests/test_line_records_emul.py in a process of its own with IRDM_LIB
pointing at an emulated build.
Usage: python line_records_emul_run.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                         # noqa: E402
import line_records                 # noqa: E402


def main():
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    print("RESULT " + json.dumps(dict(compared=line_records.check(line_records.records()))))


if __name__ == "__main__":
    main()
