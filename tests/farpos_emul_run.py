"""TEST INFRASTRUCTURE: the far-position cases of tests/test_gpu_farpos.py on the CPU emulation of the product (started by
tests/test_farpos_emul.py in a process of its own with IRDM_LIB pointing at the emulated build: tests/emul_build.py for the
pipeline, tests/resample_emul_build.py for the front ends).  Usage: python farpos_emul_run.py <case>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                      # noqa: E402
import test_gpu_farpos as G      # noqa: E402

FS = 2_000_000


def main():
    case = sys.argv[1]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {}
    if case in ("31", "32", "44", "52"):
        for form in ("whole", "lookahead"):
            res[form] = G.run_case(FS, int(case), form)[2]
    elif case == "10mhz":
        # (the register-resident decimator: the only reader of FirGeom.ring_pos / stale_pos)
        res["10mhz"] = G.run_case(10_000_000, 32, "lookahead")[2]
    elif case == "packed":
        res["packed"] = G.run_case(FS, 32, "lookahead", packed=True)[2]
    elif case == "two_hops":
        res["two_hops"] = G.run_case(FS, 32, "lookahead", two_hops=True)[2]
    elif case == "state":
        G.test_state_after_the_run(FS)
    elif case == "limit":
        res["limit"] = G.check_limit(FS)
    elif case == "frontend":
        # (2^17 + 12345 samples: 2^32 is 65536 samples behind the largest multiple of 65536 M below it for both)
        n = (1 << 17) + 12345
        for name in ("K0_D5", "K0r_25_24"):
            for power, r in ((32, 12345), (40, 0)):
                res["%s_%d_%d" % (name, power, r)] = G.check_frontend(name, irdm.FMT_CI8 if r else irdm.FMT_CF32, power, r, n=n)
        G.check_seek_refusals()
    else:
        raise SystemExit("unknown case")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
