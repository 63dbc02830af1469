"""TEST INFRASTRUCTURE: stage C alone on the designed frames of tests/stage_c_cases.py, the product on the CPU emulation
against the oracle.  Started by tests/test_stage_c_emul.py in a process of its own with IRDM_LIB pointing at the emulated
build.  Usage: python stage_c_emul_run.py <use_gardner>"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                         # noqa: E402
import stage_c_cases as sc          # noqa: E402


def main():
    gardner = int(sys.argv[1])
    assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
    res = dict(coverage=sc.coverage())
    cs = sc.cases()
    frames, dirs = [c.iq for c in cs], [c.direction for c in cs]
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768 * 4, max_bursts_per_chunk=64, use_gardner=gardner)
    try:
        t = time.time()
        # both sides on the host's libm: bit for bit, LLRs and total_phase included
        res.update(sc.run(p, gardner, exact=True))
        full = p.qpsk_demod_batch(frames, dirs)
        # position in the batch, and what lies behind num_samples in a row
        rev = p.qpsk_demod_batch(frames[::-1], dirs[::-1])[::-1]
        pad = p.qpsk_demod_batch(frames, dirs, pad=1e30)
        for c, a, b, d in zip(cs, full, rev, pad):
            assert bytes(a) == bytes(b), "%s: the record depends on the frame's position in the batch" % c.name
            assert bytes(a) == bytes(d), "%s: the record depends on what lies behind num_samples" % c.name
        res["packed_symbol_counts"] = sorted(sc.run_packed(p, 1, full) | sc.run_packed(p, 0, full))
        res["seconds"] = round(time.time() - t, 2)
    finally:
        p.close()
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
