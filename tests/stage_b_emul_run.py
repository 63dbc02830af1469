"""TEST INFRASTRUCTURE: stage B alone on the designed burst windows of tests/stage_b_cases.py, the product on the CPU
emulation against the oracle.  Started by tests/test_stage_b_emul.py in a process of its own with IRDM_LIB pointing at the
emulated build.  Usage: python stage_b_emul_run.py <sample rate> <fir_order> [option=value ...]"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                         # noqa: E402
import stage_b_cases as sb          # noqa: E402


def main():
    fs, order = int(sys.argv[1]), int(sys.argv[2])
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    p = irdm.Pipeline(fs, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64)
    try:
        p.set_option("fir_order", order)
        for kv in sys.argv[3:]:
            k, v = kv.split("=")
            p.set_option(k, int(v))
        sb.windows(fs)
        t = time.time()
        res = sb.run(p, fs, order)
        res["seconds"] = round(time.time() - t, 2)
    finally:
        p.close()
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
