"""TEST INFRASTRUCTURE: the I/Q imbalance feature (csrc/iq_moments.hpp, csrc/iq_balance.hpp) on the CPU emulation against
the numpy model of tests/balance_model.py.  Started by tests/test_balance_emul.py in a process of its own with IRDM_LIB
pointing at an emulated build.
Usage: python balance_emul_run.py balance | refusals | moments | pipeline <depth> | wire <depth> <format> | stream_moments <depth>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                         # noqa: E402
import balance_checks as bc         # noqa: E402


def main():
    case, args = sys.argv[1], [int(a) for a in sys.argv[2:]]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {"balance": bc.balance_kernel_cases, "refusals": lambda: dict(formats=bc.balance_refusal_cases()),
           "moments": bc.moments_kernel_cases, "pipeline": bc.pipeline_case, "wire": bc.wire_case,
           "stream_moments": bc.moments_case}[case](*args)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
