"""TEST INFRASTRUCTURE: the band-select front end on the CPU emulation (tests/_build/libirdm_emul_fe.so,
tests/frontend_emul_build.py) against the plain C model (tests/frontend_model.c), bit for bit.  Started by
tests/test_frontend_emul.py in a process of its own with IRDM_LIB pointing at the emulated build.
Usage: python frontend_emul_run.py <case>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import frontend_model as fm     # noqa: E402
import irdm                     # noqa: E402

Q_LIST = (0, 14418, -9000, 32767, -32767, -32768)


def stage_vs_model(fs_in, fmt, D, q, x, feeds_list):
    shift = q * fs_in / 65536.0
    st = fm.Stage(fs_in, fmt, D, shift)
    assert fm.quantise(shift, fs_in) == q
    taps = st.fe.taps()
    st.close()
    want = fm.run(x, fmt, D, q, taps)
    for feeds in feeds_list:
        st = fm.Stage(fs_in, fmt, D, shift)
        got = st.run(x, feeds)
        st.close()
        assert len(got) == len(want), (len(got), len(want))
        if not fm.same_bits(got, want):
            bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
            raise AssertionError("fmt %d D %d q %d feeds %s...: %d outputs differ, first at %d: %r vs %r" %
                                 (fmt, D, q, feeds[:4], len(bad), bad[0], got[bad[0]], want[bad[0]]))
    return len(want)


def main():
    case = sys.argv[1]
    assert "libirdm_emul_fe" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {}
    if case == "matrix":
        # five formats x the D list x the shifts, one stream whole and in ragged feeds
        for D in fm.D_LIST:
            fs_in = 2_000_000 * D
            for fmt in fm.FORMATS:
                n = 4096 * D + 777
                x = fm.random_capture(fmt, n, seed=100 * D + fmt)
                for q in Q_LIST:
                    nt = irdm.Frontend(fs_in, fmt, D, 0.0).ntaps
                    feeds = [[n]] if q not in (0, 14418) else [[n], fm.ragged_feeds(n, nt, (997,))]
                    res["%s_D%d_q%d" % (fm.NAMES[fmt], D, q)] = stage_vs_model(fs_in, fmt, D, q, x, feeds)
    elif case == "blocks":
        # one stream per D: whole, in blocks of 32768 D samples, ragged -- the same bytes
        for D in fm.D_LIST:
            fs_in = 2_000_000 * D
            n = 2 * 32768 * D + 1234
            x = fm.random_capture(irdm.FMT_CF32, n, seed=7 + D)
            nt = irdm.Frontend(fs_in, irdm.FMT_CF32, D, 0.0).ntaps
            res["D%d" % D] = stage_vs_model(fs_in, irdm.FMT_CF32, D, -14418, x,
                                            [[n], fm.block_feeds(n, 32768 * D), fm.ragged_feeds(n, nt, (9973, 30011))])
    elif case == "compose":
        # the feeder in front of the emulated pipeline (2 MHz behind a 10 MHz ci8 capture) against the oracle on the model
        import orc
        import parity
        import siggen
        fs_in, D, shift = 10_000_000, 5, 2_200_000.0
        n = int(0.75 * fs_in) // 32768 * 32768 + 4321
        q = fm.quantise(shift, fs_in)
        applied = q * fs_in / 65536.0
        rng = np.random.default_rng(5)
        bursts = [dict(start=int((0.56 + 0.045 * k) * fs_in), freq_hz=applied + siggen.channel_freq(3 * k - 4),
                       payload=list(rng.integers(0, 4, 150))) for k in range(4)]
        iq, _ = siggen.make_stream(fs_in, n, bursts, seed=9)
        x = siggen.to_ci8(iq)
        fe = irdm.Frontend(fs_in, irdm.FMT_CI8, D, shift)
        taps = fe.taps()
        fe.close()
        y = fm.run(x, irdm.FMT_CI8, D, q, taps)
        ref = orc.run_stream(y, fs_in // D, center_frequency=1622000000.0 + applied)
        for name, depth, feeds, chunk in (("depth0_whole", 0, [n], 65536 * 4), ("depth1_ragged", 1, fm.block_feeds(n, 300001), 65536),
                                          ("depth0_small", 0, fm.block_feeds(n, 100003), 32768)):
            got, app = fm.run_composed(x, fs_in, irdm.FMT_CI8, D, shift, feeds, depth, chunk)
            assert app == applied
            assert got["n_samples"] == len(y), (got["n_samples"], len(y))
            res[name] = parity.compare(got, ref)
    elif case == "float64":
        # the model against a float64 evaluation of the same formula on the same float taps and table.  Bound per component:
        # the fp32 dot product's gamma_n with one rounding per fused multiply-add (n = ntaps), plus the roundings of the
        # rotation (each component of r is two rounded products and a rounded sum: at most 3 more), with slack to 8.
        for D in fm.D_LIST:
            fs_in = 2_000_000 * D
            for fmt in fm.FORMATS:
                fe = irdm.Frontend(fs_in, fmt, D, 0.0)
                taps = fe.taps()
                fe.close()
                n = 8192 * D + 55
                x = fm.random_capture(fmt, n, seed=3 * D + fmt)
                for q in (0, 14418, -32768):
                    y = fm.run(x, fmt, D, q, taps).astype(np.complex128)
                    y64 = fm.run_float64(x, fmt, D, q, taps)
                    xf = fm.to_float(x, fmt)
                    # |r| <= sqrt(2) max|component| for either component of a rotated sample
                    xmax = np.sqrt(2.0) * max(np.abs(xf.real).max(), np.abs(xf.imag).max())
                    bound = (len(taps) + 8) * 2.0 ** -24 * np.abs(taps.astype(np.float64)).sum() * xmax
                    err = max(np.abs(y.real - y64.real).max(), np.abs(y.imag - y64.imag).max())
                    print("float64 %s D %d q %d: err %.3e bound %.3e" % (fm.NAMES[fmt], D, q, err, bound))
                    assert err <= bound, (fm.NAMES[fmt], D, q, err, bound)
                    res["%s_D%d_q%d" % (fm.NAMES[fmt], D, q)] = [float(err), float(bound)]
    elif case == "taps":
        # pass-band ripple over |f| <= 0.42 fs_out and attenuation over |f| >= 0.58 fs_out from the library's taps, 2^18-point FFT
        for D in fm.D_LIST:
            fs_in = 2_000_000 * D
            fe = irdm.Frontend(fs_in, irdm.FMT_CF32, D, 0.0)
            taps = fe.taps()
            assert len(taps) == fe.ntaps and fe.out_rate == fs_in // D
            fe.close()
            res["D%d" % D] = dict(ntaps=len(taps), **fm.response(taps, D))
    else:
        raise SystemExit("unknown case")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
