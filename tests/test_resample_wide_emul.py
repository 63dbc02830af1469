"""The front end's wide-ratio kernel K0w (csrc/resample_wide.hip, csrc/resample_wide.cpp) without a GPU: the product's
sources on the HIP emulation (tests/resample_wide_emul_build.py), driven by tests/resample_wide_emul_run.py in a process of
its own.  The assertions are those of tests/resample_wide_cases.py, which tests/test_gpu_resample_wide.py makes on the GPU:
the kernel equals the plain C restatement of the arithmetic contract (tests/resample_model.c) bit for bit at ratios beyond
125/768, K0w = K0r where both apply, and a recording whose clock runs 0.25 % fast decodes whole behind 400/401."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import resample_wide_cases as wc
import resample_wide_emul_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emul_lib():
    return resample_wide_emul_build.build()


def run_case(lib, case, timeout=3600, want_stderr=False):
    env = dict(os.environ, IRDM_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(HERE, "resample_wide_emul_run.py"), case], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return (json.loads(line[7:]), p.stderr) if want_stderr else json.loads(line[7:])


@pytest.mark.parametrize("pair", sorted(wc.PAIRS), ids=lambda p: "%d_%d" % p)
def test_kernel_equals_model_bit_for_bit(emul_lib, pair):
    """ci8, cf32, sc16q11 x q = 0, 14418, -32768: the stream whole and in ragged feeds; tiles of 2048 outputs (256 at
    100/801), more than three of them, m mod L wrapping inside a tile"""
    res = run_case(emul_lib, "pair_%d_%d" % pair)
    assert len(res) == 9 and all(v > 3 * wc.PAIRS[pair][3] for v in res.values()), res


def test_wide_equals_rational_where_both_apply(emul_lib):
    res = run_case(emul_lib, "shared")
    assert set(res) == {"%d/%d" % p for p in wc.SHARED}


def test_nan_and_inf_samples_reach_the_models_outputs_only(emul_lib):
    res = run_case(emul_lib, "nonfinite")
    assert set(res) == {"I", "Q"} and all(v > 0 for v in res.values())


def test_behind_a_seek_past_2_to_44(emul_lib):
    res = run_case(emul_lib, "seek")
    assert set(res) == {"cf32", "ci8"}


def test_create_resampler_hands_over_or_uses_k0w(emul_lib):
    assert run_case(emul_lib, "resampler")["outputs"] > 0


def test_create_resampler_refuses_what_no_kernel_does(emul_lib):
    """L = 4099; M / L above and below its range; equal rates; an output rate the pipeline refuses -- each by its own message"""
    res, err = run_case(emul_lib, "refusals", want_stderr=True)
    assert set(res) == {name for name, _, _ in wc.REFUSALS} and all(v == "refused" for v in res.values()), res
    said = {part.split("\n", 1)[0]: part.split("\n", 1)[1] for part in err.split("CASE ")[1:]}
    for name, _, message in wc.REFUSALS:
        assert message in said[name], (name, said[name])


def test_saved_band_cf32_is_the_models_bytes(emul_lib):
    assert run_case(emul_lib, "save")["bytes"] > 0


def test_off_clock_recording_decodes_behind_400_401(emul_lib):
    """Eight bursts generated at 10 025 000 S/s.  The oracle alone: on the float64-resampled stream it finds all eight,
    whole; fed at 10.025 MS/s as it is, at least one payload is not whole (the reason for the feature).  K0w's output on
    the scene is the model's, and the oracle on it returns every frame it finds on the float64 stream, every bit right."""
    res = run_case(emul_lib, "scene")
    print(res)
    assert res["ref_frames"] == res["ref_whole"] == res["expected"] == 8, res
    assert res["native_whole"] < res["expected"], res
    assert res["every_ref_frame"] and res["whole"] == 8, res


def test_the_ratio_call_needs_no_device(emul_lib):
    """irdm_frontend_resampler_ratio and irdm_frontend_wide_geometry straight from the library: kernel numbers, tile sizes"""
    L = C.CDLL(emul_lib)
    l, m, k = C.c_int(0), C.c_int(0), C.c_int(-1)
    for (fi, fo), want in (((50_000_000, 10_000_000), (1, 5, 0)), ((11_200_000, 10_000_000), (25, 28, 1)),
                           ((10_025_000, 10_000_000), (400, 401, 2)), ((8_010_000, 1_000_000), (100, 801, 2))):
        assert L.irdm_frontend_resampler_ratio(fi, fo, C.byref(l), C.byref(m), C.byref(k)) == 0
        assert (l.value, m.value, k.value) == want
    assert L.irdm_frontend_resampler_ratio(11_200_000, 9_999_999, C.byref(l), C.byref(m), C.byref(k)) == -1
    for pair, (fi, fo, _, tile) in wc.PAIRS.items():
        nt, b, lds, wg = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.irdm_frontend_wide_geometry(fi, fo, C.byref(nt), C.byref(b), C.byref(lds), C.byref(wg)) == 0
        assert b.value == tile and nt.value % 2 == 1 and nt.value <= 1 << 20 and lds.value * wg.value <= 160 * 1024, pair
