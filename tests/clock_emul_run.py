"""TEST INFRASTRUCTURE: the symbol clock estimator (csrc/symbol_clock.hpp) on the CPU emulation against tests/clock_model.py.
Started by tests/test_clock_emul.py in a process of its own with IRDM_LIB pointing at an emulated build.
Usage: python clock_emul_run.py <case>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import clock_checks as cc           # noqa: E402
import clock_model as cm            # noqa: E402
import irdm                         # noqa: E402
import siggen                       # noqa: E402


def stage():
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64, pipeline_depth=0)
    try:
        return cc.stage_cases(p)        # (batches of 65 frames: two calls' worth of max_bursts_per_chunk 64)
    finally:
        p.close()


def context():
    """a 2 MHz stream with the option on at depth 0 and depth 1 in ragged feeds, packed and full records: the same clock
    records, the summary their histogram; the option set back to 0: no records; a group refuses the option"""
    fs = 2_000_000
    iq, _ = siggen.standard_scene(fs, 3 * fs // 4, 6, 5)
    n = len(iq)
    st0, c0, d0, s0 = cc.context_run(iq, fs, [n], 0)
    rec = cc.check_summary(st0, c0)
    assert len(rec) >= 4 and st0.frames_used >= 4, (len(rec), st0.frames_used)
    assert abs(st0.median) < 2e-3 and st0.implied_rate_hz == 250000.0 * 8 * (1 + st0.median)
    st1, c1, d1, _ = cc.context_run(iq, fs, cc.ragged3(n), 1, packed=True)
    assert c1.tobytes() == c0.tobytes() and bytes(st1) == bytes(st0)
    _, c2, d2, s2 = cc.context_run(iq, fs, [n], 0, options=(("symbol_clock", 1), ("symbol_clock", 0)))
    assert len(c2) == 0 and d2.tobytes() == d0.tobytes() and s2 == s0
    cc.group_refuses()
    return dict(frames=len(rec), used=int(st0.frames_used), median=st0.median)


def main():
    case = sys.argv[1]
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {"stage": stage, "context": context}[case]()
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
