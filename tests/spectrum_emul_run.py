"""TEST INFRASTRUCTURE: option "spectrum_frames" on the CPU emulation (tests/_build/libirdm_emul_fe.so, built by
tests/frontend_emul_build.py from the product's own sources), 2 MHz (2048-point frames) and 1 MHz (1024).  Started by
tests/test_spectrum_emul.py in a process of its own with IRDM_LIB pointing at the emulated build; the checks themselves are
tests/spectrum_checks.py's, shared with tests/test_gpu_spectrum.py.  Usage: python spectrum_emul_run.py <case>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import irdm                     # noqa: E402
import reset_checks as rc       # noqa: E402
import spectrum_checks as sc    # noqa: E402

FS = 2_000_000
FS_SMALL = 1_000_000
CF32, CI8 = irdm.FMT_CF32, irdm.FMT_CI8


def main():
    case = sys.argv[1]
    assert "libirdm_emul_fe" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {}
    x = sc.scene(FS)
    if case == "values":
        # 1. R = 1, 7, 64 and more than the stream has: row count, headers, values against the oracle's plane
        res["2mhz_cf32"] = sc.check_values(FS, CF32, x, depth=1)
        res["2mhz_ci8"] = sc.check_values(FS, CI8, rc.as_format(x, CI8), depth=0, parts=3)
        res["1mhz_cf32"] = sc.check_values(FS_SMALL, CF32, sc.scene(FS_SMALL), depth=3)
    elif case == "cuts":
        # 2. one chunk, five parts, single feed blocks: the same bytes; pipeline_depth 0, 1 and 3, cf32 and ci8, detect_only
        for depth in (0, 1, 3):
            for fmt, name in ((CF32, "cf32"), (CI8, "ci8")):
                res["depth%d_%s" % (depth, name)] = sc.check_cuts(FS, fmt, rc.as_format(x, fmt), depth)
        res["detect_only"] = sc.check_cuts(FS, CF32, x, 1, options={"detect_only": 1})
        # rows of several summation groups (64 + 64 + 22 frames), the chunk boundaries inside the groups
        res["R150"] = sc.check_cuts(FS, CF32, x, 3, R=150)
        res["1mhz"] = sc.check_cuts(FS_SMALL, CF32, sc.scene(FS_SMALL), 1, R=150)
    elif case == "polls":
        # 3. rows polled after every feed + those after the flush == one poll at the end
        for depth in (0, 3):
            res["depth%d" % depth] = sc.check_mid_stream_polls(FS, CF32, x, depth)
    elif case == "records":
        # 4. the record queues with the option on == with it off
        res["depth0_full"] = sc.check_records_unchanged(FS, CF32, x, 0, rc.FULL)
        res["depth3_packed"] = sc.check_records_unchanged(FS, CI8, rc.as_format(x, CI8), 3, rc.PACKED)
    elif case == "reset":
        # 5. A with rows unpolled, reset, B == a fresh context's B; the option refused mid-stream, taken again after the reset
        b = sc.scene(FS, seed=9, n_bursts=4)
        for depth in (0, 3):
            res["depth%d" % depth] = sc.check_reset(FS, CF32, x, b, depth)
    elif case == "errors":
        # 6. values out of range; a member of a group, directly and through irdm_group_set_option
        res["range"] = sc.check_option_range(FS)
        g = irdm.Group(FS, 1, max_chunk_samples=32768 * 8)
        try:
            L = irdm.lib()
            res["group_member"] = L.irdm_set_option(g.member(0), b"spectrum_frames", 16)
            res["group"] = L.irdm_group_set_option(g.g, b"spectrum_frames", 16)
            assert res["group_member"] == -1 and res["group"] == -1, res
        finally:
            g.close()
    else:
        raise SystemExit("unknown case")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
