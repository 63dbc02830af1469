"""TEST INFRASTRUCTURE: irdm_reset / irdm_frontend_reset on the CPU emulation (tests/_build/libirdm_emul_fe.so: the whole
product, front end included, built by tests/frontend_emul_build.py from the product's own sources), 2 MHz.  Started by
tests/test_reset_emul.py in a process of its own with IRDM_LIB pointing at the emulated build; the checks themselves are
tests/reset_checks.py's, shared with tests/test_gpu_reset.py.  Usage: python reset_emul_run.py <case>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                     # noqa: E402
import reset_checks as rc       # noqa: E402

FS = 2_000_000


def main():
    case = sys.argv[1]
    assert "libirdm_emul_fe" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {}
    if case != "frontend":
        a32, b32 = rc.dirty_scene(FS), rc.plain_scene(FS)
    if case == "matrix":
        # 1. A (dirty), flush, poll, reset, B == B on a fresh context: pipeline_depth 0, 1 and 2 (fed in place with
        #    look-ahead), cf32 and ci8, full records and packed + parsed + frame records
        for depth, parts_a, parts_b in ((0, 2, 1), (1, 3, 4), (2, 5, 4)):
            for fmt, name in ((irdm.FMT_CF32, "cf32"), (irdm.FMT_CI8, "ci8")):
                a, b = rc.as_format(a32, fmt), rc.as_format(b32, fmt)
                for opts, oname in ((rc.FULL, "full"), (rc.PACKED, "packed")):
                    res["depth%d_%s_%s" % (depth, name, oname)] = rc.check_reuse(FS, fmt, depth, opts, a, b, parts_a, parts_b)
    elif case == "mid_stream":
        # 2. the reset after A's first chunk (which holds the squelch wave), records unpolled: the queues hold B's only
        for depth, parts_a in ((0, 2), (2, 2), (2, 5)):
            for opts, oname in ((rc.FULL, "full"), (rc.PACKED, "packed")):
                res["depth%d_%dparts_%s" % (depth, parts_a, oname)] = rc.check_reuse(FS, irdm.FMT_CF32, depth, opts, a32, b32, parts_a, 4,
                                                                                      mid_stream=True)
    elif case == "states":
        # 3. + 5. the exported detector state right after the reset and after B; A, B, A: the second A equals the first
        for depth, parts_a, parts_b in ((0, 2, 2), (2, 5, 4)):
            res["depth%d" % depth] = rc.check_reuse(FS, irdm.FMT_CF32, depth, rc.FULL, a32, b32, parts_a, parts_b, states=True, thrice=True)
    elif case == "oracle":
        # 4. B's records behind the reset against the oracle's
        for depth, parts_b in ((0, 1), (2, 4)):
            res["depth%d" % depth] = rc.check_oracle(FS, depth, b32, parts_b, a32)
    elif case == "refused":
        # 6. irdm_reset between irdm_feed_begin and irdm_feed_end: -1, and the stream goes on to the fresh context's result;
        #    a member of a group refuses too
        for depth, parts_b in ((0, 2), (1, 4)):
            res["depth%d" % depth] = rc.check_reuse(FS, irdm.FMT_CF32, depth, rc.PACKED, a32, b32, 3, parts_b, refused=True)
        g = irdm.Group(FS, 1, max_chunk_samples=32768 * 8)
        try:
            res["group_member"] = irdm.lib().irdm_reset(g.member(0), rc.CF_B, rc.T0_B)
            assert res["group_member"] == -1
        finally:
            g.close()
    elif case == "frontend":
        # 7. run A (ending on a partial block); finish; reset; run B == a fresh front end's B
        for D, fmt in ((2, irdm.FMT_CI8), (5, irdm.FMT_CF32)):
            res["D%d" % D] = rc.check_frontend(2_000_000 * D, D, fmt)
    else:
        raise SystemExit("unknown case")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
