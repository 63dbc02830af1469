"""TEST INFRASTRUCTURE: IRDM_FMT_CU8 end to end on the CPU emulation (tests/emul_build.py; the front-end cases on the
builds of tests/frontend_emul_build.py and tests/resample_emul_build.py).  Every run equals the emulated cf32 context on
the converted samples record for record and bit for bit, and the oracle on the converted stream under the parity rules
(tests/parity.py).  Started by tests/test_cu8_emul.py in a process of its own with IRDM_LIB pointing at the emulated build.
Usage: python cu8_emul_run.py <case>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import cu8                  # noqa: E402
import formats16 as f16     # noqa: E402
import irdm                 # noqa: E402


def check(u, fs, **kw):
    """the cu8 context vs the cf32 context on the converted samples (bitwise) and the oracle"""
    import orc
    import parity
    y = cu8.converted(u)
    got = f16.run(u, fs, irdm.FMT_CU8, **kw)
    n = f16.same_records(got, f16.run(y, fs, irdm.FMT_CF32, **kw))
    s = parity.compare(got, orc.run_stream(y, fs))
    s["records"] = n
    return s


def stage_pair(make_stage, u, feeds_list):
    """the band of the cu8 capture = the band of the cf32 capture of the converted samples, bit for bit, for every cut"""
    import frontend_model as fm
    y = cu8.converted(u)
    st = make_stage(irdm.FMT_CF32)
    want = st.run(y, [len(y)])
    st.close()
    assert len(want) > 0
    for feeds in feeds_list:
        st = make_stage(irdm.FMT_CU8)
        got = st.run(u, feeds)
        st.close()
        assert fm.same_bits(got, want), (feeds[:4], len(got), len(want))
    return len(want)


def main():
    case = sys.argv[1]
    res = {}
    if case == "2mhz":
        # 2048-point frames (the generic K1), the any-M decimator (M = 20): its general path reads through burst_sample
        assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
        fs = 2_000_000
        u = cu8.cu8_scene(fs, 1.2, 6, seed=162)
        n = len(u) // 2
        res["whole"] = check(u, fs)
        res["chunked_depth1"] = check(u, fs, chunks=f16.chunks_of(n, 4), depth=1)
        res["sequential_scan"] = check(u, fs, options={"scan_mode": 1})
    elif case == "12mhz":
        # 16384-point frames (K1 p32<14>), the register-resident decimator at M = 48, two chunks
        assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
        fs = 12_000_000
        u = cu8.cu8_scene(fs, 0.85, 3, seed=12)
        res["two_chunks_depth1"] = check(u, fs, chunks=f16.chunks_of(len(u) // 2, 2), depth=1)
    elif case == "k0":
        # K0 at D = 5 with a shift: whole and in ragged feeds
        import frontend_model as fm
        assert "libirdm_emul_fe" in irdm.LIB_PATH or "libirdm_emul_rs" in irdm.LIB_PATH, irdm.LIB_PATH
        fs_in, D = 10_000_000, 5
        n = 4096 * D + 777
        u = np.random.default_rng(65).integers(0, 256, 2 * n, dtype=np.uint8)
        shift = 14418 * fs_in / 65536.0
        nt = irdm.Frontend(fs_in, irdm.FMT_CU8, D, 0.0).ntaps
        res["outputs"] = stage_pair(lambda fmt: fm.Stage(fs_in, fmt, D, shift), u, [[n], fm.ragged_feeds(n, nt, (997,))])
        for bad in (5, 7):
            try:
                irdm.Frontend(fs_in, bad, D, 0.0)
            except RuntimeError:
                res["refused_%d" % bad] = True
    elif case == "k0r":
        # K0r, 2.4 -> 2.5 MS/s (25/24), with a shift: whole and in ragged feeds
        import frontend_model as fm
        import resample_model as rm
        assert "libirdm_emul_rs" in irdm.LIB_PATH, irdm.LIB_PATH
        fi, fo = 2_400_000, 2_500_000
        n = 24 * 700 + 321
        u = np.random.default_rng(66).integers(0, 256, 2 * n, dtype=np.uint8)
        shift = -9000 * fi / 65536.0
        fe = irdm.Frontend.rational(fi, irdm.FMT_CU8, fo, 0.0)
        nt, L = fe.ntaps, fe.ratio[0]
        fe.close()
        res["outputs"] = stage_pair(lambda fmt: rm.Stage(fi, fmt, fo, shift), u, [[n], rm.ragged_feeds(n, nt, L, (997,))])
        for bad in (5, 7):
            try:
                irdm.Frontend.rational(fi, bad, fo, 0.0)
            except RuntimeError:
                res["refused_%d" % bad] = True
    else:
        raise SystemExit("unknown case")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
