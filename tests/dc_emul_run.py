"""TEST INFRASTRUCTURE: the DC tracker (csrc/dc_block.hpp) on the CPU emulation against the numpy model of tests/dc_model.py.
Started by tests/test_dc_emul.py in a process of its own with IRDM_LIB pointing at an emulated build.
Usage: python dc_emul_run.py kernel | refusals | carry | pipeline <depth> | wire <depth> | composition <depth>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                         # noqa: E402
import dc_checks as dc              # noqa: E402


def main():
    case, args = sys.argv[1], [int(a) for a in sys.argv[2:]]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {"kernel": dc.kernel_cases, "refusals": lambda: dict(formats=dc.refusal_cases()), "carry": dc.carry_case,
           "pipeline": dc.pipeline_case, "wire": dc.wire_case, "composition": dc.composition_case}[case](*args)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
