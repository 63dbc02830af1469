"""TEST INFRASTRUCTURE: exchanged I and Q (csrc/iq_swap.hpp, iq_sense_kernel of csrc/bitlayer.hip) on the CPU emulation
against numpy and tests/iq_sense_model.py.  Started by tests/test_iq_emul.py in a process of its own with IRDM_LIB pointing
at an emulated build.
Usage: python iq_emul_run.py swap | votes | pipeline <depth> <format> | random <depth>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import iq_checks as ic              # noqa: E402
import irdm                         # noqa: E402


def votes():
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64, pipeline_depth=0)
    try:
        return ic.check_votes(p)        # (several launches' worth of max_bursts_per_chunk 64)
    finally:
        p.close()


def main():
    case, args = sys.argv[1], [int(a) for a in sys.argv[2:]]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {"swap": lambda: dict(cases=ic.swap_cases()), "votes": votes, "pipeline": ic.pipeline_case,
           "random": ic.random_payloads_case}[case](*args)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
