"""TEST INFRASTRUCTURE: the corrections of the host feeds together (tests/hostchain_checks.py) on the CPU emulation, context and
front end.  Started by tests/test_hostchain_emul.py in a process of its own with IRDM_LIB pointing at the emulated build of
tests/frontend_emul_build.py.
Usage: python hostchain_emul_run.py context | context_prime | front_end | front_end_prime | refusals"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                         # noqa: E402
import hostchain_checks as hc       # noqa: E402


def main():
    assert "libirdm_emul_fe" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {"context": hc.context_cases, "context_prime": hc.context_prime_case, "front_end": hc.front_end_cases,
           "front_end_prime": hc.front_end_prime_case, "refusals": hc.refusal_cases}[sys.argv[1]]()
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
