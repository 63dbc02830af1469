"""The front end's rational mode (csrc/resample.hip, csrc/resample.cpp, the L / M bookkeeping of csrc/frontend.cpp) without a
GPU: the product's sources on the HIP emulation (tests/resample_emul_build.py), driven by tests/resample_emul_run.py in a
process of its own.  The kernel equals the plain C restatement of the arithmetic contract (tests/resample_model.c) bit for
bit; the model with L = 1 is the integer front end's; it stays inside the derived fp32 bound of a float64 evaluation; the
prototype meets the stated response; resampling is what makes an off-grid capture demodulate; the feeder composes with the
pipeline."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import frontend_model as fm
import irdm
import resample_emul_build
import resample_model as rm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emul_lib():
    return resample_emul_build.build()


def run_case(lib, case, timeout=3600, want_stderr=False):
    env = dict(os.environ, IRDM_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(HERE, "resample_emul_run.py"), case], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return (json.loads(line[7:]), p.stderr) if want_stderr else json.loads(line[7:])


def test_kernel_equals_model_all_pairs_formats_shifts(emul_lib):
    """seven ratios x five formats x q zero / positive / negative / +-32768, each with the stream whole and in ragged feeds
    of 1, a prime, and one less than the taps of a phase"""
    res = run_case(emul_lib, "matrix")
    assert len(res) == len(rm.PAIRS) * 5 * 6
    assert all(v > 1000 for v in res.values())


def test_kernel_equals_model_other_ratios_reset_and_integer(emul_lib):
    """ratios whose L is no multiple of 5 (8-phase blocks), odd M; the same bits after irdm_frontend_reset following a dirty
    run; an integer ratio gives the integer front end"""
    res = run_case(emul_lib, "other_ratios")
    assert set(res) == {"2/3", "6/7", "4/9", "8/9", "reset", "integer"}
    assert all(v > 0 for v in res.values())


def test_create_refuses_what_it_cannot_do(emul_lib):
    """L > 125; M > 768 with L <= 125; M / L above, below and equal to 1; an output rate the pipeline refuses (rational and
    integer); an unknown format; a shift beyond half the capture rate -- each refused, each by its own message"""
    res, err = run_case(emul_lib, "refusals", want_stderr=True)
    assert set(res) == {name for name, _, _ in rm.REFUSALS} and all(v == "refused" for v in res.values()), res
    said = {part.split("\n", 1)[0]: part.split("\n", 1)[1] for part in err.split("CASE ")[1:]}
    for name, _, message in rm.REFUSALS:
        assert message in said[name], (name, said[name])


def test_model_with_l_1_is_the_integer_front_end():
    """rs_model_run at L = 1, M = D on K0's taps = fe_model_run at D, bit for bit"""
    for D in (2, 5, 16):
        fs_in = 2_000_000 * D
        taps = fm.design_taps(fs_in, D)
        for fmt, q in ((irdm.FMT_CI8, 14418), (irdm.FMT_CF32, -32768), (irdm.FMT_SC16Q11, 0)):
            x = fm.random_capture(fmt, 4096 * D + 777, seed=D + fmt)
            assert fm.same_bits(rm.run(x, fmt, 1, D, q, taps), fm.run(x, fmt, D, q, taps)), (D, fmt)


def test_named_rates_are_exact_and_l_1_design_is_k0s():
    """L * in_rate is exactly representable as the float the designer takes, for every pair the README names; the design
    at L = 1 gives K0's taps"""
    for fi, fo in rm.NAMED:
        L, M = rm.ratio(fi, fo)
        assert L <= 125 and M <= 768 and 24 * L <= 25 * M <= 16 * 25 * L
        assert int(np.float32(L * fi)) == L * fi, (fi, fo)
    for D in (2, 5, 16):
        assert np.array_equal(rm.design_taps(2_000_000 * D, 2_000_000).view(np.uint32), fm.design_taps(2_000_000 * D, D).view(np.uint32))


def test_model_within_fp32_bound_of_float64():
    """per output |y - y64| <= (Tp + 8) 2^-24 sum|P_phase| max|r| per component, Tp the taps of the output's phase: the fp32
    dot product's gamma_n with one rounding per fused multiply-add, plus the roundings of the rotation (at most 3), with
    slack to 8 -- the integer front end's bound, per branch"""
    for (L, M), (fi, fo) in rm.PAIRS.items():
        taps = rm.design_taps(fi, fo)
        sums = rm.phase_tap_sums(taps, L, M)
        for fmt in fm.FORMATS:
            n = 40 * M + 55
            x = fm.random_capture(fmt, n, seed=3 * L + M + fmt)
            xf = fm.to_float(x, fmt)
            xmax = np.sqrt(2.0) * max(np.abs(xf.real).max(), np.abs(xf.imag).max())
            for q in (0, 14418, -32768):
                y = rm.run(x, fmt, L, M, q, taps).astype(np.complex128)
                y64 = rm.run_float64(x, fmt, L, M, q, taps)
                ph = np.arange(len(y)) % L
                bound = np.array([(sums[r][0] + 8) * 2.0 ** -24 * sums[r][1] * xmax for r in range(L)])[ph]
                err = np.maximum(np.abs(y.real - y64.real), np.abs(y.imag - y64.imag))
                worst = int(np.argmax(err / bound))
                print("float64 %s %d/%d q %d: worst err %.3e of bound %.3e" % (fm.NAMES[fmt], L, M, q, err[worst], bound[worst]))
                assert np.all(err <= bound), (fm.NAMES[fmt], L, M, q, err[worst], bound[worst])


def test_prototype_meets_the_stated_response(emul_lib):
    """at the rate L in_rate: >= 80 dB down from 0.58 f_min to half that rate, <= 0.002 dB of ripple up to 0.42 f_min after
    removing the gain L; the library's taps are the oracle's restatement of the design, bit for bit"""
    res = run_case(emul_lib, "taps")
    assert set(res) == {"%d/%d" % k for k in rm.PAIRS}
    for name, r in res.items():
        print("%s: %d taps, ripple %.5f dB, attenuation %.2f dB" % (name, r["ntaps"], r["ripple_db"], r["atten_db"]))
        assert r["atten_db"] >= 80.0, (name, r)
        assert r["ripple_db"] <= 0.002, (name, r)
        assert r["ntaps"] % 2 == 1


@pytest.mark.parametrize("name", sorted(rm.SCENES))
def test_off_grid_capture_needs_the_resampler(name):
    """The reason for the feature, model -> oracle.  Eight bursts spaced in time, within 0.40 f_min of the centre, amp 0.05.
    (a) fed at the capture rate, the oracle returns no payload whole (the reference alone); (b) through the model, every
    payload is the leading hard bits of exactly one frame, and there is nothing else."""
    import orc
    s = rm.SCENES[name]
    x, expect = rm.offgrid_scene(name)
    assert len(expect) >= 6
    L, M = rm.ratio(s["in_rate"], s["out_rate"])
    native = orc.run_stream(x, s["in_rate"])
    print("%s native: %d frames, %d whole" % (name, len(native.demods), rm.whole_payloads(native.demods, expect)))
    assert rm.whole_payloads(native.demods, expect) == 0
    y = rm.run(x, irdm.FMT_CF32, L, M, 0, rm.design_taps(s["in_rate"], s["out_rate"]))
    ref = orc.run_stream(y, s["out_rate"])
    fm.check_scene_demods(ref.demods, expect)


def test_feeder_composes_with_the_pipeline(emul_lib):
    """irdm_frontend_feed_host + irdm_frontend_flush of a rational front end in front of the emulated pipeline (depth 0 and
    1, ragged feeds) against the oracle run on the model's output, under tests/parity.py's rules"""
    res = run_case(emul_lib, "compose")
    assert set(res) == {"depth0_whole", "depth1_ragged", "depth0_small"}
    for name, s in res.items():
        assert s["bursts"] >= 6 and s["demods"] >= 6 and s["whole"] == s["expected"] == 8, (name, s)


def test_config_struct_layout_matches_the_header(tmp_path):
    """irdm_frontend_rational_config_t: sizeof and every offset as gcc lays the header's struct out"""
    names = [n for n, _ in irdm.FrontendRationalConfig._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "irdm_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(irdm_frontend_rational_config_t));\n' +
                   "".join('    printf(" %%zu", offsetof(irdm_frontend_rational_config_t, %s));\n' % n for n in names) +
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(irdm.FrontendRationalConfig)] + [getattr(irdm.FrontendRationalConfig, n).offset for n in names]
    hdr = open(os.path.join(ROOT, "include", "irdm_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} irdm_frontend_rational_config_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == names == ["device", "in_rate", "in_format", "out_rate", "shift_hz"]
