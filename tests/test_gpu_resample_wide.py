"""The front end's wide-ratio kernel K0w on the GPU (csrc/resample_wide.hip, csrc/resample_wide.cpp): the assertions of
tests/resample_wide_cases.py -- the kernel against the plain C model bit for bit at ratios beyond 125/768, K0w = K0r where
both apply, non-finite samples, a seek past 2^44, irdm_frontend_create_resampler and its refusals, the saved band -- and, end
to end, a recording whose clock runs 0.25 % fast: what --clock-check says about it and what --resample-to then makes of it."""
import os
import subprocess

import numpy as np
import pytest

import frontend_model as fm
import irdm
import orc
import parity
import resample_model as rm
import resample_wide_cases as wc

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")


@pytest.mark.parametrize("pair", sorted(wc.PAIRS), ids=lambda p: "%d_%d" % p)
def test_kernel_equals_model_bit_for_bit(pair):
    """ci8, cf32, sc16q11 x q = 0, 14418, -32768: the stream whole and in ragged feeds; tiles of 2048 outputs (256 at
    100/801), more than three of them, m mod L wrapping inside a tile"""
    for fmt in wc.FORMATS:
        for q in wc.Q_LIST:
            assert wc.check_pair(pair, fmt, q) > 3 * wc.PAIRS[pair][3]


@pytest.mark.parametrize("pair", sorted(wc.SHARED), ids=lambda p: "%d_%d" % p)
def test_wide_equals_rational_where_both_apply(pair):
    wc.check_shared(pair)


def test_nan_and_inf_samples_reach_the_models_outputs_only():
    counts = wc.check_nonfinite()
    print("non-finite outputs:", counts)


def test_behind_a_seek_past_2_to_44():
    wc.check_seek()


def test_create_resampler_hands_over_or_uses_k0w():
    wc.check_resampler()


def test_create_resampler_refuses_what_no_kernel_does(capfd):
    """L = 4099; M / L above and below its range; equal rates; an output rate the pipeline refuses -- each by its own message"""
    for name, args, message in wc.REFUSALS:
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            irdm.Frontend.resampler(*args)
        assert message in capfd.readouterr().err, name
        assert irdm.Frontend.resampler_ratio(args[0], args[2]) is None or name == "out_rate"
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        irdm.Frontend.wide(50_000_000, irdm.FMT_CI8, 10_000_000)
    assert "integer ratio 1/5" in capfd.readouterr().err


def test_saved_band_cf32_is_the_models_bytes():
    wc.check_save_band()


@pytest.fixture(scope="module")
def scene():
    """the 10.025 MS/s scene as a ci8 capture, the model's output at 10 MS/s, the float64 evaluation of the same formula,
    and the oracle's records on both"""
    s = wc.SCENE
    x, expect = wc.scene(irdm.FMT_CI8)
    fe = irdm.Frontend.resampler(s["in_rate"], irdm.FMT_CI8, s["out_rate"])
    taps, ratio = fe.taps(), fe.ratio
    fe.close()
    assert ratio == (400, 401)
    y = rm.run(x, irdm.FMT_CI8, 400, 401, 0, taps)
    y64 = wc.float64_resample(fm.to_float(x, irdm.FMT_CI8), 400, 401, taps)
    return dict(x=x, expect=expect, y=y, ref=orc.run_stream(y, s["out_rate"]), ref64=orc.run_stream(y64, s["out_rate"]))


@pytest.mark.parametrize("depth,feed,chunk", [(0, "host", 1 << 20), (3, "device", 1 << 19)])
def test_off_clock_recording_behind_400_401(scene, depth, feed, chunk):
    """irdm_frontend_feed_* + flush of irdm_frontend_create_resampler's object in front of a cf32 context: the oracle's
    records on the model's output (tests/parity.py's rules), and every frame the oracle finds on the float64-resampled
    stream, every payload bit right"""
    s = wc.SCENE
    n = len(scene["x"]) // 2
    step = chunk * 401 // 400
    feeds = fm.block_feeds(n, step) if feed == "host" else fm.block_feeds(n, step - 12347)
    got, applied = wc.run_composed(scene["x"], s["in_rate"], irdm.FMT_CI8, s["out_rate"], 0.0, feeds, depth, chunk, feed=feed)
    assert applied == 0.0 and got["n_samples"] == len(scene["y"])
    parity.compare(got, scene["ref"])
    found = [e for e in scene["expect"] if rm.whole_payloads(scene["ref64"].demods, [e])]
    print("float64 stream: %d frames, %d of %d payloads whole" % (len(scene["ref64"].demods), len(found), len(scene["expect"])))
    assert len(found) == len(scene["ref64"].demods) == len(scene["expect"]) == 8
    assert rm.whole_payloads(got["demods"], found) == len(found)
    assert wc.frames_whole(got["demods"], scene["ref64"].demods)


def test_off_clock_recording_fed_as_it_is_loses_frames(scene):
    """the same capture fed to a context at 10.025 MS/s: at least one frame is not whole"""
    s = wc.SCENE
    iq, expect = wc.scene()
    got = parity.run_gpu(iq, s["in_rate"])
    whole = rm.whole_payloads(got["demods"], expect)
    print("native at 10.025 MS/s: %d frames, %d whole" % (len(got["demods"]), whole))
    assert whole < len(expect)


def test_cli_clock_check_names_the_remedy_and_the_remedy_works(scene, tmp_path):
    """-r 10000000 --clock-check prints the clause with --resample-to 10000000; -r 10025000 --resample-to 10000000
    --clock-check -v exits 0, prints the (400/401) line and a clock: line with no clause"""
    s = wc.SCENE
    cap = tmp_path / "cap.ci8"
    scene["x"].tofile(str(cap))
    common = [EXE, "-f", str(cap), "-c", "1622000000", "--file-info", "rw", "--chunk", str(1 << 20), "--start-time", "1700000000"]
    a = subprocess.run(common + ["-r", str(s["out_rate"]), "--clock-check"], capture_output=True, timeout=600)
    assert a.returncode == 0, a.stderr.decode()[-2000:]
    line = [l for l in a.stderr.decode().splitlines() if l.startswith("clock: ")][-1]
    assert line.endswith("-- the samples look like 10025000 S/s, not 10000000: check -r, or --resample-to 10000000"), line
    b = subprocess.run(common + ["-r", str(s["in_rate"]), "--resample-to", str(s["out_rate"]), "--clock-check", "-v"],
                       capture_output=True, timeout=600)
    assert b.returncode == 0, b.stderr.decode()[-2000:]
    err = b.stderr.decode()
    assert "front end: 10025000 -> 10000000 samples/s (400/401), %d taps" % irdm.Frontend.wide_geometry(s["in_rate"], s["out_rate"])["ntaps"] in err, err[-2000:]
    line = [l for l in err.splitlines() if l.startswith("clock: ")][-1]
    assert " -- " not in line and "frames; symbol clock" in line, line
    assert b.stdout.count(b"RAW: ") == len(scene["expect"])
