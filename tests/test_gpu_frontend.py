"""The band-select front end on the GPU (csrc/frontend.hip, csrc/frontend.cpp): the kernel against the plain C model bit for
bit, the feeder in front of the pipeline against the oracle run on the model's output (tests/parity.py's rules: burst
indices, downmixed samples and hard bits exact, soft outputs within 1e-4), the signal scene, and the command line."""
import os
import subprocess

import numpy as np
import pytest

import frontend_model as fm
import irdm
import orc
import parity

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")


@pytest.mark.parametrize("D", fm.D_LIST)
def test_kernel_equals_model_bit_for_bit(D):
    """irdm_frontend_run_device / _finish_device on 2^24 + 12345 input samples, five formats, whole and in ragged feeds
    (1, ntaps - 1, primes): every output bit of tests/frontend_model.c"""
    fs_in = 2_000_000 * D
    n = (1 << 24) + 12345
    for fmt in fm.FORMATS:
        q = (14418, -9000, 32767, -32768, 0)[fmt]
        shift = q * fs_in / 65536.0
        x = fm.random_capture(fmt, n, seed=1000 * D + fmt)
        st = fm.Stage(fs_in, fmt, D, shift)
        taps = st.fe.taps()
        assert np.array_equal(taps.view(np.uint32), fm.design_taps(fs_in, D).view(np.uint32))
        got = st.run(x, fm.ragged_feeds(n, len(taps), (999983, 65537, 2000003, 7 * 32768 * D)))
        st.close()
        want = fm.run(x, fmt, D, q, taps)
        assert fm.same_bits(got, want), (fm.NAMES[fmt], D, int((got.view(np.uint64) != want.view(np.uint64)).sum())
                                         if len(got) == len(want) else (len(got), len(want)))
        if fmt == irdm.FMT_CF32:
            st = fm.Stage(fs_in, fmt, D, shift)
            whole = st.run(x, [n])
            st.close()
            assert fm.same_bits(whole, want)


@pytest.fixture(scope="module")
def scene():
    """the wideband scene, the model's output and the oracle's records on it (tests/test_frontend_emul.py checks the
    scene's selection on the CPU)"""
    x, expect, q = fm.wideband_scene()
    s = fm.SCENE
    fe = irdm.Frontend(s["fs_in"], irdm.FMT_CI8, s["D"], s["shift_hz"])
    taps = fe.taps()
    applied = fe.applied_shift_hz
    fe.close()
    assert applied == q * s["fs_in"] / 65536.0
    y = fm.run(x, irdm.FMT_CI8, s["D"], q, taps)
    ref = orc.run_stream(y, s["fs_in"] // s["D"], center_frequency=1622000000.0 + applied)
    return dict(x=x, expect=expect, q=q, y=y, ref=ref, applied=applied)


@pytest.mark.parametrize("depth,feed,chunk", [(0, "host", 1 << 20), (3, "host", 1 << 20), (3, "device", 1 << 19), (0, "device", 1 << 21)])
def test_feeder_and_pipeline_equal_the_oracle_on_the_model(scene, depth, feed, chunk):
    """irdm_frontend_feed_* + irdm_frontend_flush in front of a cf32 context (depth 0: scratch chunk; depth 3: converted in
    place into the history ring) -- the same bar as every other input path -- and the scene's payloads, all of them, nothing else"""
    s = fm.SCENE
    n = len(scene["x"]) // 2
    feeds = fm.block_feeds(n, s["D"] * chunk) if feed == "host" else fm.block_feeds(n, s["D"] * chunk - 12347)
    got, applied = fm.run_composed(scene["x"], s["fs_in"], irdm.FMT_CI8, s["D"], s["shift_hz"], feeds, depth, chunk, feed=feed)
    assert applied == scene["applied"]
    assert got["n_samples"] == len(scene["y"])
    summary = parity.compare(got, scene["ref"])
    assert summary["demods"] == s["n_inband"], summary
    fm.check_scene_demods(got["demods"], scene["expect"])


def test_cli_band_select_prints_what_the_model_file_prints(scene, tmp_path):
    """--band-center / --decimate on the 50 MHz ci8 file = the binary on the model's cf32 file at 10 MHz with -c at the
    band centre and the same --file-info"""
    s = fm.SCENE
    wide = tmp_path / "wide.ci8"
    scene["x"].tofile(str(wide))
    narrow = tmp_path / "narrow.cf32"
    scene["y"].tofile(str(narrow))
    capture_center = 1615000000.0
    band = capture_center + s["shift_hz"]
    a = subprocess.run([EXE, "-f", str(wide), "-r", str(s["fs_in"]), "-c", "%.3f" % capture_center, "--band-center", "%.3f" % band,
                        "--decimate", str(s["D"]), "--file-info", "fe", "--chunk", str(1 << 20), "-v"],
                       capture_output=True, timeout=600)
    assert a.returncode == 0, a.stderr.decode()[-2000:]
    assert b"front end: 50000000 -> 10000000 samples/s, 223 taps" in a.stderr
    b = subprocess.run([EXE, "-f", str(narrow), "-r", str(s["fs_in"] // s["D"]), "-c", "%.17g" % (capture_center + scene["applied"]),
                        "--file-info", "fe", "--chunk", str(1 << 20)], capture_output=True, timeout=600)
    assert b.returncode == 0, b.stderr.decode()[-2000:]
    assert a.stdout.count(b"RAW: ") == s["n_inband"]
    # A file-mode run stamps its frames from the wall clock at its start (burst_detect.c:849-853), so two runs of the binary
    # cannot agree in the time field itself (tests/test_gpu_parsed.py compares CLI runs the same way): every other byte is
    # compared, and the time field relative to the run's first line -- the positions of the output samples at fs_out --
    # to the last printed digit (0.1 us; one unit for the two roundings).
    la, lb = (o.decode().splitlines() for o in (a.stdout, b.stdout))
    assert [l.split(" ")[:2] + l.split(" ")[3:] for l in la] == [l.split(" ")[:2] + l.split(" ")[3:] for l in lb]
    ta, tb = ([float(l.split(" ")[2]) for l in ls] for ls in (la, lb))
    assert all(abs((x - ta[0]) - (y - tb[0])) <= 0.00021 for x, y in zip(ta, tb)), (ta, tb)
    assert ta[-1] - ta[0] > 200.0          # (ms: the scene's bursts are 45 ms apart)
    # one flag without the other, and a group behind a front end: usage errors
    for extra in (["--decimate", "5"], ["--band-center", "1626000000"], ["--band-center", "1626000000", "--decimate", "5", "--gpus", "2"]):
        r = subprocess.run([EXE, "-f", str(wide), "-r", str(s["fs_in"])] + extra, capture_output=True, timeout=120)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)


def test_cli_without_the_flags_still_refuses_a_wideband_rate(tmp_path):
    """unchanged behaviour: a 30.72 MHz file without the flags ends with the unsupported-rate message (which now names the way out)"""
    f = tmp_path / "x.ci8"
    f.write_bytes(b"\0" * 2 * 65536)
    r = subprocess.run([EXE, "-f", str(f), "-r", "30720000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "irdm_hip: unsupported sample rate 30720000 (fft_size 32768)" in r.stderr
    assert "--band-center / --decimate" in r.stderr and "irdm_frontend_create" in r.stderr
    assert r.stdout == ""


def test_create_refuses_what_it_cannot_do():
    for args in ((50_000_000, irdm.FMT_CI8, 1), (50_000_000, irdm.FMT_CI8, 17), (50_000_000, irdm.FMT_CI8, 3),
                 (50_000_000, 7, 5), (61_440_000, irdm.FMT_CI16, 2)):
        with pytest.raises(RuntimeError):
            irdm.Frontend(*args)
    with pytest.raises(RuntimeError):
        irdm.Frontend(50_000_000, irdm.FMT_CI8, 5, shift_hz=26e6)
    fe = irdm.Frontend(61_440_000, irdm.FMT_SC16Q11, 6, shift_hz=-3e6)
    assert fe.out_rate == 10_240_000 and abs(fe.applied_shift_hz + 3e6) <= 61_440_000 / 65536 / 2
    fe.close()
