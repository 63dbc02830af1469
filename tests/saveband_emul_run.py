"""TEST INFRASTRUCTURE: saving the band (irdm_requantize_device, irdm_frontend_save) on the CPU emulation
(tests/_build/libirdm_emul_fe.so, or libirdm_emul_rs.so for the rational case) against the numpy model
(tests/saveband_model.py), byte for byte.  Started by tests/test_saveband_emul.py in a process of its own with IRDM_LIB
pointing at the emulated build.
Usage: python saveband_emul_run.py <case>"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import frontend_model as fm     # noqa: E402
import irdm                     # noqa: E402
import saveband_model as sm     # noqa: E402

CASES = ((irdm.FMT_CI8, 2.0), (irdm.FMT_CI16, 0.37), (irdm.FMT_CF32, 1.0))
FS_IN, D, Q, SLOT = 4_000_000, 2, 14418, 4099


def main():
    case = sys.argv[1]
    assert "libirdm_emul_" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {}
    shift = Q * FS_IN / 65536.0
    if case == "kernel":
        res["calls"] = sm.check_kernel()
    elif case == "stage":
        # D = 2 at 4 MS/s, ci8 and cf32 captures, whole and in ragged feeds, pieces of 4099 samples
        n = (1 << 18) + 12345
        for fmt in (irdm.FMT_CI8, irdm.FMT_CF32):
            x = fm.random_capture(fmt, n, seed=40 + fmt)
            fe = irdm.Frontend(FS_IN, fmt, D, shift)
            taps = fe.taps()
            fe.close()
            want_y = fm.run(x, fmt, D, Q, taps)
            res[fm.NAMES[fmt]] = sm.check_saved(lambda: fm.Stage(FS_IN, fmt, D, shift), x, want_y,
                                                [[n], fm.ragged_feeds(n, len(taps))], CASES, SLOT)
    elif case == "rational":
        # 11.2 -> 10 MS/s (25 / 28)
        import resample_model as rm
        fi, fo = 11_200_000, 10_000_000
        L, M = rm.ratio(fi, fo)
        assert (L, M) == (25, 28)
        n = 2 * (900 * M + 777)
        q = fm.quantise(150e3, fi)
        sh = q * fi / 65536.0
        x = fm.random_capture(irdm.FMT_CI8, n, seed=28)
        taps = rm.design_taps(fi, fo)
        want_y = rm.run(x, irdm.FMT_CI8, L, M, q, taps)
        assert len(want_y) == rm.n_outputs(n, L, M)
        res["25/28"] = sm.check_saved(lambda: rm.Stage(fi, irdm.FMT_CI8, fo, sh), x, want_y,
                                      [[n], rm.ragged_feeds(n, len(taps), L, (9973,))], CASES, SLOT)
    elif case == "props":
        n = 40000
        x = fm.random_capture(irdm.FMT_CI8, n, seed=3)
        x2 = fm.random_capture(irdm.FMT_CI8, n + 777, seed=4)
        st = fm.Stage(FS_IN, irdm.FMT_CI8, D, shift)
        taps = st.fe.taps()
        want_y = fm.run(x, irdm.FMT_CI8, D, Q, taps)
        # saving off: today's outputs
        assert fm.same_bits(st.run(x, [n]), want_y)
        st.fe.reset()
        # a reset mid-stream (pieces outstanding, nothing flushed), then a second stream: its bytes and statistics alone
        st.fe.save(irdm.FMT_CI8, gain=2.0, slot_samples=SLOT)
        d_out = irdm.lib().irdm_device_alloc(0, 8 * n)
        d_in = irdm.device_buffer(x)
        assert irdm.lib().irdm_frontend_run_device(st.fe.h, C.c_void_p(d_in), n, C.c_void_p(d_out), n, None) > 0
        first = len(b"".join(st.fe.saved))
        assert 0 < first < 2 * len(want_y)
        st.fe.reset()
        del st.fe.saved[:]
        y2 = st.run(x2, fm.ragged_feeds(n + 777, len(taps)))
        want2 = fm.run(x2, irdm.FMT_CI8, D, Q, taps)
        wbytes, wstats = sm.quantise(want2, irdm.FMT_CI8, 2.0)
        assert fm.same_bits(y2, want2) and b"".join(st.fe.saved) == wbytes and sm.same_stats(st.fe.save_stats(), wstats)
        res["reset"] = [first, len(wbytes)]
        # mid-stream (finished, not reset): refused; after a reset: accepted, NULL turns it off and the outputs stay
        try:
            st.fe.save(irdm.FMT_CI16)
            raise AssertionError("irdm_frontend_save on a finished stream was accepted")
        except RuntimeError:
            pass
        st.fe.reset()
        assert irdm.lib().irdm_frontend_run_device(st.fe.h, C.c_void_p(d_in), 1, C.c_void_p(d_out), n, None) == 0
        try:
            st.fe.save(irdm.FMT_CI16)
            raise AssertionError("irdm_frontend_save after the first sample was accepted")
        except RuntimeError:
            pass
        st.fe.reset()
        st.fe.save(None)
        assert fm.same_bits(st.run(x, fm.ragged_feeds(n, len(taps))), want_y)
        st.fe.reset()
        # bad fields
        for fmt, gain in ((irdm.FMT_CI16_FULL, 1.0), (irdm.FMT_CI8, 0.0), (irdm.FMT_CI8, -1.0), (irdm.FMT_CI8, float("inf")),
                          (irdm.FMT_CI8, float("nan")), (irdm.FMT_CF32, 2.0), (irdm.FMT_CI16, 3e38)):
            try:
                st.fe.save(fmt, gain=gain)
                raise AssertionError("irdm_frontend_save took format %d gain %r" % (fmt, gain))
            except RuntimeError:
                pass
        # a sink that returns non-zero: the call in progress returns -1
        seen = []
        st.fe.save(irdm.FMT_CI8, sink=lambda b: seen.append(len(b)) or len(seen) >= 2, slot_samples=SLOT)
        rc = irdm.lib().irdm_frontend_run_device(st.fe.h, C.c_void_p(d_in), n, C.c_void_p(d_out), n, None)
        assert rc == -1 and len(seen) == 2, (rc, seen)
        res["stop"] = seen
        irdm.device_free(d_in)
        irdm.lib().irdm_device_free(d_out)
        st.close()
    else:
        raise SystemExit("unknown case")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
