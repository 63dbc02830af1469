"""The front end's rational mode on the GPU (csrc/resample.hip, csrc/resample.cpp): the kernel against the plain C model bit
for bit, the feeder in front of the pipeline against the oracle run on the model's output (tests/parity.py's rules), the
off-grid scene -- whole payloads behind the resampler, none without it -- the command line and the create call's refusals."""
import os
import subprocess

import numpy as np
import pytest

import frontend_model as fm
import irdm
import orc
import parity
import resample_model as rm
import reset_checks as rc

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")


@pytest.mark.parametrize("pair", sorted(rm.PAIRS), ids=lambda p: "%d_%d" % p)
def test_kernel_equals_model_bit_for_bit(pair):
    """irdm_frontend_run_device / _finish_device of a rational front end on 2^24 + 12345 input samples, five formats: the
    stream whole on a fresh object; in ragged feeds (1, one less than the taps of a phase, primes) on another; and once
    again, ragged, on that object after irdm_frontend_reset following its dirty run: every output bit of
    tests/resample_model.c"""
    L, M = pair
    fi, fo = rm.PAIRS[pair]
    n = (1 << 24) + 12345
    for fmt in fm.FORMATS:
        q = (14418, -9000, 32767, -32768, 0)[fmt]
        shift = q * fi / 65536.0
        x = fm.random_capture(fmt, n, seed=1000 * L + M + fmt)
        st = rm.Stage(fi, fmt, fo, shift)
        assert st.fe.ratio == (L, M) and st.fe.out_rate == fo
        taps = st.fe.taps()
        assert np.array_equal(taps.view(np.uint32), rm.design_taps(fi, fo).view(np.uint32))
        want = rm.run(x, fmt, L, M, q, taps)
        whole = st.run(x, [n])
        st.close()
        assert fm.same_bits(whole, want), (fm.NAMES[fmt], pair, "whole", int((whole.view(np.uint64) != want.view(np.uint64)).sum())
                                           if len(whole) == len(want) else (len(whole), len(want)))
        feeds = rm.ragged_feeds(n, len(taps), L, (999983, 65537, 2000003, 7 * 32768 * 5))
        st = rm.Stage(fi, fmt, fo, shift)
        got = st.run(x, feeds)
        assert fm.same_bits(got, want), (fm.NAMES[fmt], pair, "ragged", int((got.view(np.uint64) != want.view(np.uint64)).sum())
                                         if len(got) == len(want) else (len(got), len(want)))
        st.reset()                                   # (finished, with a carried tail and counts: a dirty object)
        again = st.run(x, feeds[::-1])
        st.close()
        assert fm.same_bits(again, want), (fm.NAMES[fmt], pair, "ragged after reset")


@pytest.fixture(scope="module")
def scene():
    """the 11.2 MS/s scene (tests/test_resample_emul.py checks its selection on the CPU), the model's output at 10 MS/s and
    the oracle's records on it"""
    s = rm.SCENES["11.2->10"]
    x, expect = rm.offgrid_scene("11.2->10", irdm.FMT_CI8)
    shift = 150_000.0
    fe = irdm.Frontend.rational(s["in_rate"], irdm.FMT_CI8, s["out_rate"], shift)
    taps, applied, ratio = fe.taps(), fe.applied_shift_hz, fe.ratio
    fe.close()
    q = fm.quantise(shift, s["in_rate"])
    assert applied == q * s["in_rate"] / 65536.0 and ratio == (25, 28)
    y = rm.run(x, irdm.FMT_CI8, 25, 28, q, taps)
    ref = orc.run_stream(y, s["out_rate"], center_frequency=1622000000.0 + applied)
    return dict(x=x, expect=expect, q=q, y=y, ref=ref, applied=applied, shift=shift)


@pytest.mark.parametrize("depth,feed,chunk", [(0, "host", 1 << 20), (3, "host", 1 << 20), (3, "device", 1 << 19), (0, "device", 1 << 21)])
def test_feeder_and_pipeline_equal_the_oracle_on_the_model(scene, depth, feed, chunk):
    """irdm_frontend_feed_* + irdm_frontend_flush of the rational front end in front of a cf32 context -- the same bar as
    every other input path -- and the scene's payloads, all of them, nothing else"""
    s = rm.SCENES["11.2->10"]
    n = len(scene["x"]) // 2
    step = chunk * 28 // 25
    feeds = fm.block_feeds(n, step) if feed == "host" else fm.block_feeds(n, step - 12347)
    got, applied = rm.run_composed(scene["x"], s["in_rate"], irdm.FMT_CI8, s["out_rate"], scene["shift"], feeds, depth, chunk, feed=feed)
    assert applied == scene["applied"]
    assert got["n_samples"] == len(scene["y"])
    summary = parity.compare(got, scene["ref"])
    assert summary["demods"] == len(scene["expect"]) == 8, summary
    fm.check_scene_demods(got["demods"], scene["expect"])


def test_without_the_resampler_no_payload_is_whole(scene):
    """the same capture fed to a context at 11.2 MS/s: frames are found, no payload comes out whole"""
    s = rm.SCENES["11.2->10"]
    iq, expect = rm.offgrid_scene("11.2->10")
    got = parity.run_gpu(iq, s["in_rate"])
    print("native at 11.2 MS/s: %d frames, %d whole" % (len(got["demods"]), rm.whole_payloads(got["demods"], expect)))
    assert len(got["demods"]) >= 6
    assert rm.whole_payloads(got["demods"], expect) == 0


def test_cli_resample_prints_what_the_model_file_prints(scene, tmp_path):
    """--resample-to 10000000 (with --band-center) on the 11.2 MS/s ci8 file = the binary on the model's cf32 file at 10 MHz
    with -c at the band centre and the same --file-info"""
    s = rm.SCENES["11.2->10"]
    wide = tmp_path / "cap.ci8"
    scene["x"].tofile(str(wide))
    narrow = tmp_path / "narrow.cf32"
    scene["y"].tofile(str(narrow))
    cc = 1621000000.0
    a = subprocess.run([EXE, "-f", str(wide), "-r", str(s["in_rate"]), "-c", "%.3f" % cc, "--band-center", "%.3f" % (cc + scene["shift"]),
                        "--resample-to", str(s["out_rate"]), "--file-info", "rs", "--chunk", str(1 << 20), "-v"],
                       capture_output=True, timeout=600)
    assert a.returncode == 0, a.stderr.decode()[-2000:]
    assert b"front end: 11200000 -> 10000000 samples/s (25/28), 1245 taps" in a.stderr, a.stderr.decode()[-2000:]
    b = subprocess.run([EXE, "-f", str(narrow), "-r", str(s["out_rate"]), "-c", "%.17g" % (cc + scene["applied"]),
                        "--file-info", "rs", "--chunk", str(1 << 20)], capture_output=True, timeout=600)
    assert b.returncode == 0, b.stderr.decode()[-2000:]
    assert a.stdout.count(b"RAW: ") == len(scene["expect"])
    # (two runs of the binary stamp their frames from their own wall clocks: every other byte is compared, and the time
    # field relative to the run's first line, as tests/test_gpu_frontend.py compares its pair)
    la, lb = (o.decode().splitlines() for o in (a.stdout, b.stdout))
    assert [l.split(" ")[:2] + l.split(" ")[3:] for l in la] == [l.split(" ")[:2] + l.split(" ")[3:] for l in lb]
    ta, tb = ([float(l.split(" ")[2]) for l in ls] for ls in (la, lb))
    assert all(abs((x - ta[0]) - (y - tb[0])) <= 0.00021 for x, y in zip(ta, tb)), (ta, tb)
    assert ta[-1] - ta[0] > 150.0


def test_cli_resample_at_an_integer_ratio_is_decimate(tmp_path):
    """--resample-to 10000000 on the 50 MS/s scene of tests/frontend_model.py = --decimate 5, byte for byte, under a fixed
    --start-time"""
    s = fm.SCENE
    x, _, _ = fm.wideband_scene()
    wide = tmp_path / "wide.ci8"
    x.tofile(str(wide))
    cc = 1615000000.0
    common = [EXE, "-f", str(wide), "-r", str(s["fs_in"]), "-c", "%.3f" % cc, "--band-center", "%.3f" % (cc + s["shift_hz"]),
              "--file-info", "fe", "--chunk", str(1 << 20), "--start-time", "1700000000"]
    a = subprocess.run(common + ["--decimate", str(s["D"])], capture_output=True, timeout=600)
    b = subprocess.run(common + ["--resample-to", str(s["fs_in"] // s["D"])], capture_output=True, timeout=600)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr.decode()[-1000:], b.stderr.decode()[-1000:])
    assert a.stdout.count(b"RAW: ") == s["n_inband"]
    assert a.stdout == b.stdout


def test_cli_batch_behind_the_resampler(scene, tmp_path):
    """two recordings in one run (one front end, one context, irdm_frontend_reset between them) = the two single runs"""
    s = rm.SCENES["11.2->10"]
    n = len(scene["x"]) // 2
    files = []
    for i, c in enumerate((n, int(0.60 * s["in_rate"]) + 12345)):
        path = str(tmp_path / ("cap%d.ci8" % i))
        scene["x"][:2 * c].tofile(path)
        files.append(path)
    common = ["-r", s["in_rate"], "-c", "1621000000", "--resample-to", s["out_rate"], "--file-info", "rs", "--chunk", 1 << 20]
    res = rc.check_cli_batch(EXE, str(tmp_path), files, ["1700000000", "1700003600.25"], common, [[]])
    assert all(v > 0 for v in res["raw"]), res


def test_cli_refusals(tmp_path):
    """--decimate beside it, --gpus 2, a ratio outside the limits (L, M / L), HZ equal to -r: exit 2, nothing on stdout"""
    f = tmp_path / "x.ci8"
    f.write_bytes(b"\0" * 2 * 65536)
    for extra in (["--resample-to", "10000000", "--decimate", "5", "--band-center", "1626000000"],
                  ["--resample-to", "10000000", "--gpus", "2"], ["--resample-to", "9999999"], ["--resample-to", "12000000"],
                  ["--resample-to", "500000"], ["--resample-to", "11200000"]):
        r = subprocess.run([EXE, "-f", str(f), "-r", "11200000"] + extra, capture_output=True, timeout=120)
        assert r.returncode == 2 and r.stdout == b"", (extra, r.returncode, r.stderr)


def test_create_refuses_what_it_cannot_do(capfd):
    """L > 125; M > 768 with L <= 125; M / L outside 24/25 .. 16; the capture's own rate; an unsupported output rate; an
    unknown format; a shift beyond half the capture rate -- each by its own message; an integer ratio gives the integer
    front end"""
    for name, args, message in rm.REFUSALS:
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            irdm.Frontend.rational(*args)
        assert message in capfd.readouterr().err, name
    fe = irdm.Frontend.rational(61_440_000, irdm.FMT_SC16Q11, 10_000_000, shift_hz=-3e6)
    assert fe.ratio == (125, 768) and fe.out_rate == 10_000_000 and abs(fe.applied_shift_hz + 3e6) <= 61_440_000 / 65536 / 2
    fe.close()
    fe = irdm.Frontend.rational(50_000_000, irdm.FMT_CI8, 10_000_000)
    assert fe.ratio == (1, 5) and fe.ntaps == 223
    fe.close()
