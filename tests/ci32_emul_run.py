"""TEST INFRASTRUCTURE: IRDM_FMT_CI32 and IRDM_FMT_CI32_24 end to end on the CPU emulation (tests/emul_build.py; the
front-end cases on the builds of tests/frontend_emul_build.py and tests/resample_emul_build.py).  Every run equals the
emulated cf32 context on the converted samples record for record and bit for bit, and the oracle on the converted stream
under the parity rules (tests/parity.py).  Started by tests/test_ci32_emul.py in a process of its own with IRDM_LIB pointing
at the emulated build.
Usage: python ci32_emul_run.py <case>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import ci32                 # noqa: E402
import formats16 as f16     # noqa: E402
import irdm                 # noqa: E402

F8, F9 = irdm.FMT_CI32, irdm.FMT_CI32_24


def check(v, fs, fmt, **kw):
    """the int32 context vs the cf32 context on the converted samples (bitwise) and the oracle"""
    import orc
    import parity
    y = ci32.converted(v, fmt)
    got = f16.run(v, fs, fmt, **kw)
    n = f16.same_records(got, f16.run(y, fs, irdm.FMT_CF32, **kw))
    s = parity.compare(got, orc.run_stream(y, fs))
    s["records"] = n
    return s


def stage_pair(make_stage, v, fmt, feeds_list):
    """the band of the int32 capture = the band of the cf32 capture of the converted samples, bit for bit, for every cut"""
    import frontend_model as fm
    y = ci32.converted(v, fmt)
    st = make_stage(irdm.FMT_CF32)
    want = st.run(y, [len(y)])
    st.close()
    assert len(want) > 0
    for feeds in feeds_list:
        st = make_stage(fmt)
        got = st.run(v, feeds)
        st.close()
        assert fm.same_bits(got, want), (feeds[:4], len(got), len(want))
    return len(want)


def capture(fmt, n, seed):
    """a capture over the format's whole range, the extreme codes among its samples"""
    v = ci32.stats_input(fmt, n, seed)
    v[100], v[101] = ci32.I32_MIN, ci32.I32_MAX
    return v


def refusals(make):
    out = {}
    for bad in (5, 7, 10):
        try:
            make(bad)
        except RuntimeError:
            out["refused_%d" % bad] = True
    return out


def main():
    case = sys.argv[1]
    res = {}
    if case == "2mhz":
        # 2048-point frames (the generic K1), the any-M decimator (M = 20): its general path reads through burst_sample
        assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
        fs = 2_000_000
        v = ci32.with_extremes(ci32.ci32_scene(fs, 1.2, 6, seed=162, fmt=F8))
        n = len(v) // 2
        x = ci32.converted(v, F8).view(np.float32)
        frac = float(np.mean(np.abs(v.astype(np.int64)) >= 2 ** 24))
        assert x[10] == -1.0 and x[11] == 1.0 and x[12] == 1.0 and x[13] == -1.0       # INT32_MAX -> exactly 1.0
        assert frac > 0.5, frac                                                        # (float)v rounds for most values
        res["whole"] = check(v, fs, F8)
        res["chunked_depth1"] = check(v, fs, F8, chunks=f16.chunks_of(n, 4), depth=1)
        res["sequential_scan"] = check(v, fs, F8, options={"scan_mode": 1})
        v9 = ci32.ci32_scene(fs, 1.2, 6, seed=162, fmt=F9)
        assert int(np.abs(v9.astype(np.int64)).max()) < 2 ** 23
        res["whole_24"] = check(v9, fs, F9)
        res["chunked_depth1_24"] = check(v9, fs, F9, chunks=f16.chunks_of(n, 4), depth=1)
        res["frac_over_24_bits"] = frac
        for bad in (5, 7, 10):
            try:
                irdm.Pipeline(fs, fmt=bad)
            except RuntimeError:
                res["refused_%d" % bad] = True
    elif case == "12mhz":
        # 16384-point frames (K1 p32<14>), the register-resident decimator at M = 48, two chunks
        assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
        fs = 12_000_000
        for fmt, key in ((F8, "two_chunks_depth1"), (F9, "two_chunks_depth1_24")):
            v = ci32.ci32_scene(fs, 0.95, 5, seed=12, fmt=fmt)
            res[key] = check(v, fs, fmt, chunks=f16.chunks_of(len(v) // 2, 2), depth=1)
    elif case == "k0":
        # K0 at D = 5 with a shift: whole and in ragged feeds
        import frontend_model as fm
        assert "libirdm_emul_fe" in irdm.LIB_PATH or "libirdm_emul_rs" in irdm.LIB_PATH, irdm.LIB_PATH
        fs_in, D = 10_000_000, 5
        n = 4096 * D + 777
        shift = 14418 * fs_in / 65536.0
        nt = irdm.Frontend(fs_in, F8, D, 0.0).ntaps
        for fmt in (F8, F9):
            res["outputs_%d" % fmt] = stage_pair(lambda f: fm.Stage(fs_in, f, D, shift), capture(fmt, n, 65 + fmt), fmt,
                                                 [[n], fm.ragged_feeds(n, nt, (997,))])
        res.update(refusals(lambda bad: irdm.Frontend(fs_in, bad, D, 0.0)))
    elif case == "k0r":
        # K0r, 2.4 -> 2.5 MS/s (25/24), with a shift: whole and in ragged feeds
        import frontend_model as fm
        import resample_model as rm
        assert "libirdm_emul_rs" in irdm.LIB_PATH, irdm.LIB_PATH
        fi, fo = 2_400_000, 2_500_000
        n = 24 * 700 + 321
        shift = -9000 * fi / 65536.0
        fe = irdm.Frontend.rational(fi, F8, fo, 0.0)
        nt, L = fe.ntaps, fe.ratio[0]
        fe.close()
        for fmt in (F8, F9):
            res["outputs_%d" % fmt] = stage_pair(lambda f: rm.Stage(fi, f, fo, shift), capture(fmt, n, 66 + fmt), fmt,
                                                 [[n], rm.ragged_feeds(n, nt, L, (997,))])
        res.update(refusals(lambda bad: irdm.Frontend.rational(fi, bad, fo, 0.0)))
    elif case == "stats":
        import ci32_stats_checks as cs
        assert "libirdm_emul" in irdm.LIB_PATH, irdm.LIB_PATH
        res = cs.all_cases()
    else:
        raise SystemExit("unknown case")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
