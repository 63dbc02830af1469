"""TEST INFRASTRUCTURE: the wide-ratio kernel K0w on the CPU emulation (tests/_build/libirdm_emul_rw.so,
tests/resample_wide_emul_build.py): the checks of tests/resample_wide_cases.py, which tests/test_gpu_resample_wide.py makes
on the GPU.  Started by tests/test_resample_wide_emul.py in a process of its own with IRDM_LIB pointing at the emulated build.
Usage: python resample_wide_emul_run.py <case>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "iridium-sniffer_amd"))

import frontend_model as fm     # noqa: E402
import irdm                     # noqa: E402
import resample_model as rm     # noqa: E402
import resample_wide_cases as wc     # noqa: E402


def main():
    case = sys.argv[1]
    assert "libirdm_emul_rw" in irdm.LIB_PATH, irdm.LIB_PATH
    res = {}
    if case.startswith("pair_"):
        pair = tuple(int(v) for v in case.split("_")[1:])
        for fmt in wc.FORMATS:
            for q in wc.Q_LIST:
                res["%s_q%d" % (fm.NAMES[fmt], q)] = wc.check_pair(pair, fmt, q)
    elif case == "shared":
        for pair in wc.SHARED:
            res["%d/%d" % pair] = wc.check_shared(pair)
    elif case == "nonfinite":
        res = wc.check_nonfinite()
    elif case == "seek":
        res = wc.check_seek()
    elif case == "resampler":
        res["outputs"] = wc.check_resampler()
    elif case == "save":
        res["bytes"] = wc.check_save_band()
    elif case == "refusals":
        # (each attempt is announced on stderr, so that the test can tell which message belongs to which)
        for name, args, _ in wc.REFUSALS:
            sys.stderr.write("CASE %s\n" % name)
            sys.stderr.flush()
            try:
                irdm.Frontend.resampler(*args).close()
                res[name] = "created"
            except RuntimeError:
                res[name] = "refused"
    elif case == "scene":
        # K0w's output on the 10.025 MS/s scene = the model's; the oracle on it finds what it finds on the float64 stream
        import orc
        s = wc.SCENE
        x, expect = wc.scene()
        st = wc.Stage(s["in_rate"], irdm.FMT_CF32, s["out_rate"])
        taps = st.fe.taps()
        got = st.run(x, fm.block_feeds(len(x), 1 << 20))
        st.close()
        assert wc.differ(got, rm.run(x, irdm.FMT_CF32, 400, 401, 0, taps)) is None
        ref = orc.run_stream(wc.float64_resample(x, 400, 401, taps), s["out_rate"])
        out = orc.run_stream(got, s["out_rate"])
        native = orc.run_stream(x, s["in_rate"])
        res = dict(expected=len(expect), ref_frames=len(ref.demods), ref_whole=rm.whole_payloads(ref.demods, expect),
                   frames=len(out.demods), whole=rm.whole_payloads(out.demods, expect), every_ref_frame=wc.frames_whole(out.demods, ref.demods),
                   native_frames=len(native.demods), native_whole=rm.whole_payloads(native.demods, expect))
    else:
        raise SystemExit("unknown case")
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
