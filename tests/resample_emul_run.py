"""TEST INFRASTRUCTURE: the front end's rational mode on the CPU emulation (tests/_build/libirdm_emul_rs.so,
tests/resample_emul_build.py) against the plain C model (tests/resample_model.c), bit for bit.  Started by
tests/test_resample_emul.py in a process of its own with IRDM_LIB pointing at the emulated build.
Usage: python resample_emul_run.py <case>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import frontend_model as fm     # noqa: E402
import irdm                     # noqa: E402
import resample_model as rm     # noqa: E402

Q_LIST = (0, 14418, -9000, 32767, -32768, 32768)


def stream_len(M):
    """more than three tiles of the kernel at every ratio (a tile is at most 256 periods of M inputs, and fewer periods
    where 256 M inputs exceed about 8192), so that a whole feed has tiles wholly inside the chunk"""
    return (900 * M if M < 64 else 220 * M) + 777


def stage_vs_model(in_rate, out_rate, fmt, q, x, feeds_list):
    L, M = rm.ratio(in_rate, out_rate)
    shift = q * in_rate / 65536.0
    assert fm.quantise(shift, in_rate) == q
    st = rm.Stage(in_rate, fmt, out_rate, shift)
    assert st.fe.ratio == (L, M) and st.fe.out_rate == out_rate
    taps = st.fe.taps()
    st.close()
    want = rm.run(x, fmt, L, M, q, taps)
    assert len(want) == rm.n_outputs(fm.n_samples(x, fmt), L, M)
    for feeds in feeds_list:
        st = rm.Stage(in_rate, fmt, out_rate, shift)
        got = st.run(x, feeds)
        st.close()
        assert len(got) == len(want), (len(got), len(want))
        if not fm.same_bits(got, want):
            bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
            raise AssertionError("fmt %d %d/%d q %d feeds %s...: %d outputs differ, first at %d: %r vs %r" %
                                 (fmt, L, M, q, feeds[:4], len(bad), bad[0], got[bad[0]], want[bad[0]]))
    return len(want)


def main():
    case = sys.argv[1]
    assert "libirdm_emul_rs" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {}
    if case == "matrix":
        # the pairs x five formats x the shifts; the stream whole and in ragged feeds
        for (L, M), (fi, fo) in rm.PAIRS.items():
            for fmt in fm.FORMATS:
                n = stream_len(M)
                x = fm.random_capture(fmt, n, seed=1000 * L + M + fmt)
                nt = len(rm.design_taps(fi, fo))
                for q in Q_LIST:
                    feeds = [[n], rm.ragged_feeds(n, nt, L, (997,))]
                    res["%s_%d/%d_q%d" % (fm.NAMES[fmt], L, M, q)] = stage_vs_model(fi, fo, fmt, q, x, feeds)
    elif case == "other_ratios":
        # ratios whose L is no multiple of 5 (the kernel's 8-phase blocks), an odd M, and a reset after a dirty run
        for fi, fo in ((3_000_000, 2_000_000), (2_800_000, 2_400_000), (27_000_000, 12_000_000), (2_250_000, 2_000_000)):
            L, M = rm.ratio(fi, fo)
            n = stream_len(M)
            x = fm.random_capture(irdm.FMT_CI16_FULL, n, seed=L + M)
            nt = irdm.Frontend.rational(fi, irdm.FMT_CI16_FULL, fo).ntaps
            res["%d/%d" % (L, M)] = stage_vs_model(fi, fo, irdm.FMT_CI16_FULL, -14418, x, [[n], rm.ragged_feeds(n, nt, L, (997,))])
        fi, fo = rm.PAIRS[(25, 24)]
        n = stream_len(24)
        x = fm.random_capture(irdm.FMT_CI8, n, seed=77)
        st = rm.Stage(fi, irdm.FMT_CI8, fo, 100e3)
        q = fm.quantise(100e3, fi)
        want = rm.run(x, irdm.FMT_CI8, 25, 24, q, st.fe.taps())
        dirty = st.run(x[:2 * 5000], [5000])          # (flushed: the object is finished, its tail and counts are dirty)
        assert len(dirty) == rm.n_outputs(5000, 25, 24)
        st.reset()
        got = st.run(x, rm.ragged_feeds(n, st.fe.ntaps, 25, (997,)))
        st.close()
        assert fm.same_bits(got, want)
        res["reset"] = len(got)
        # an integer ratio is the integer front end: K0's object, K0's output
        fe = irdm.Frontend.rational(10_000_000, irdm.FMT_CI8, 2_000_000)
        assert fe.ratio == (1, 5) and fe.ntaps == irdm.Frontend(10_000_000, irdm.FMT_CI8, 5).ntaps
        fe.close()
        res["integer"] = 1
    elif case == "refusals":
        # L > 125, M / L outside 24/25 .. 16, the same rate, an unsupported output rate, a shift beyond half the capture
        # rate, an unknown format
        # (each attempt is announced on stderr, so that the test can tell which message belongs to which)
        for name, args, _ in rm.REFUSALS:
            sys.stderr.write("CASE %s\n" % name)
            sys.stderr.flush()
            try:
                irdm.Frontend.rational(*args).close()
                res[name] = "created"
            except RuntimeError:
                res[name] = "refused"
    elif case == "taps":
        # the library's prototype = the oracle's restatement of the design; its response at the rate L in_rate
        for (L, M), (fi, fo) in rm.PAIRS.items():
            fe = irdm.Frontend.rational(fi, irdm.FMT_CF32, fo)
            taps = fe.taps()
            assert len(taps) == fe.ntaps and fe.out_rate == fo and fe.ratio == (L, M)
            fe.close()
            assert np.array_equal(taps.view(np.uint32), rm.design_taps(fi, fo).view(np.uint32))
            res["%d/%d" % (L, M)] = dict(ntaps=len(taps), **rm.response(taps, L, M))
    elif case == "compose":
        # the feeder in front of the emulated pipeline (2.5 MHz behind a 2.4 MHz ci8 capture) against the oracle on the model
        import orc
        import parity
        s = rm.SCENES["2.4->2.5"]
        fi, fo = s["in_rate"], s["out_rate"]
        L, M = rm.ratio(fi, fo)
        x, expect = rm.offgrid_scene("2.4->2.5", irdm.FMT_CI8)
        n = len(x) // 2
        shift = 30_000.0
        q = fm.quantise(shift, fi)
        applied = q * fi / 65536.0
        y = rm.run(x, irdm.FMT_CI8, L, M, q, rm.design_taps(fi, fo))
        ref = orc.run_stream(y, fo, center_frequency=1622000000.0 + applied)
        for name, depth, feeds, chunk in (("depth0_whole", 0, [n], 65536 * 4), ("depth1_ragged", 1, fm.block_feeds(n, 300001), 65536),
                                          ("depth0_small", 0, fm.block_feeds(n, 100003), 32768)):
            got, app = rm.run_composed(x, fi, irdm.FMT_CI8, fo, shift, feeds, depth, chunk)
            assert app == applied
            assert got["n_samples"] == len(y), (got["n_samples"], len(y))
            res[name] = parity.compare(got, ref)
            res[name]["whole"] = rm.whole_payloads(got["demods"], expect)
            res[name]["expected"] = len(expect)
    else:
        raise SystemExit("unknown case")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
