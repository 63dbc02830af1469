"""TEST INFRASTRUCTURE: the band scan's mid-stream declines on the CPU emulation (tests/_build/libirdm_emul.so, built by
tests/emul_build.py from the product's own sources).  Started by tests/test_decline_emul.py in a process of its own with
IRDM_LIB pointing at the emulated build; the cases and the checks are tests/decline_checks.py's, shared with
tests/test_gpu_decline.py.  Usage: python decline_emul_run.py <case> <config>[:packed] ..."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                     # noqa: E402
import decline_checks as dc     # noqa: E402


def main():
    name = sys.argv[1]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {}
    for arg in sys.argv[2:]:
        config, _, form = arg.partition(":")
        res[arg] = dc.check(name, config, packed=form == "packed")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
