"""TEST INFRASTRUCTURE: option scrub / irdm_scrub_device (csrc/scrub.hpp) on the CPU emulation against the numpy model of
tests/scrub_model.py.  Started by tests/test_scrub_emul.py in a process of its own with IRDM_LIB pointing at an emulated
build.
Usage: python scrub_emul_run.py kernel | refusals | pipeline <depth>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                         # noqa: E402
import scrub_checks as sc           # noqa: E402


def main():
    case, args = sys.argv[1], [int(a) for a in sys.argv[2:]]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {"kernel": lambda: dict(cases=sc.kernel_cases()), "refusals": lambda: dict(formats=sc.refusal_cases()),
           "pipeline": sc.pipeline_case}[case](*args)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
