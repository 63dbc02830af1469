"""TEST INFRASTRUCTURE: the front end's shared load stage on the CPU emulation (tests/_build/libirdm_emul_rw.so,
tests/resample_wide_emul_build.py: K0, K0r and K0w in one library): one row of tests/fe_stage_cases.py, which
tests/test_gpu_fe_stage.py runs on the GPU.  Started by tests/test_fe_stage_emul.py in a process of its own with IRDM_LIB
pointing at the emulated build.
Usage: python fe_stage_emul_run.py <row>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import fe_stage_cases as fc     # noqa: E402
import irdm                     # noqa: E402


def main():
    assert "libirdm_emul_rw" in irdm.LIB_PATH, irdm.LIB_PATH
    print("RESULT " + json.dumps(fc.check(sys.argv[1])))


if __name__ == "__main__":
    main()
