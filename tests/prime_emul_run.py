"""TEST INFRASTRUCTURE: irdm_prime_host (csrc/feed.cpp) on the CPU emulation against the CPU oracle run over P || x.  Started
by tests/test_prime_emul.py in a process of its own with IRDM_LIB pointing at an emulated build.
Usage: python prime_emul_run.py scene <full|excerpt> <depth> | options <depth> | side <depth>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                         # noqa: E402
import prime_checks as pc           # noqa: E402


def main():
    case, args = sys.argv[1], sys.argv[2:]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    if case == "scene":
        res = pc.scene_case(args[0], int(args[1]))
    else:
        res = {"options": pc.options_case, "side": pc.side_case}[case](int(args[0]))
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
