"""-m gpu: the binary's --burst-resample.  The 2.4 MS/s scene of tests/burst_resample_checks.py as an RTL-SDR cu8 file: with the
flag every RAW line is a whole frame, -v names the ratio and --clock-check finds the clock right; without it the output is
the oracle's, as ever.  A 61.44 MS/s ci8 capture through --band-center / --decimate 6 (10.24 MS/s behind the front end) gives
every frame whole.  A rate whose L exceeds 4096 exits 2."""
import os
import re
import subprocess

import numpy as np
import pytest

import burst_resample_checks as bc
import cu8
import frontend_model as fm
import irdm
import orc
import parity

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
FS = 2_400_000


def run_cli(args, timeout=300):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, timeout=timeout)


def bits_of_line(line):
    return [int(c) for c in parity.raw_fields(line)[8]]


@pytest.fixture(scope="module")
def rtl(tmp_path_factory):
    iq, truth = bc.scene(FS)
    u = cu8.to_cu8(iq)
    path = tmp_path_factory.mktemp("br_cli") / "scene.cu8"
    u.tofile(str(path))
    return dict(path=path, truth=truth, u=u)


def common(path):
    return ["-f", path, "-r", FS, "--format", "cu8", "--file-info", "t", "--start-time", "1700000000"]


def test_without_the_flag_the_output_is_the_oracles(rtl):
    r = run_cli(common(rtl["path"]))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    ref = orc.run_stream(cu8.converted(rtl["u"]), FS)
    lines, want = r.stdout.decode().splitlines(), [l.strip() for l in ref.raw_lines("t")]
    assert len(lines) == len(want) >= 6
    for a, b in zip(lines, want):
        fa, fb = parity.raw_fields(a), parity.raw_fields(b)
        assert fa[:2] == fb[:2] and fa[3:6] == fb[3:6] and fa[7:] == fb[7:], (a, b)
        assert abs(fa[2] - fb[2]) <= 1 and abs(fa[6] - fb[6]) <= 1e-4, (a, b)
    assert not any(bits_of_line(l) in [t["bits"] for t in rtl["truth"]] for l in lines)
    assert b"burst resample" not in r.stderr


def test_with_the_flag_every_line_is_a_whole_frame_and_the_clock_is_right(rtl):
    plain = run_cli(common(rtl["path"]))
    r = run_cli(common(rtl["path"]) + ["--burst-resample", "--clock-check", "-v"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(plain.stdout.decode().splitlines()) >= 6
    truth_bits = [t["bits"] for t in rtl["truth"]]
    for l in lines:
        assert bits_of_line(l) in truth_bits, l
    err = r.stderr.decode()
    assert err.count("burst resample: 240000 -> 250000 samples/s per burst (25/24), 20 taps per phase\n") == 1, err[-2000:]
    clock = [l for l in err.splitlines() if l.startswith("clock: ")]
    assert len(clock) == 1, err[-2000:]
    m = re.match(r"clock: (\d+) frames; symbol clock ([+-]\d+\.\d+) % \(quartiles", clock[0])
    assert m and int(m.group(1)) >= 5 and abs(float(m.group(2))) <= 0.05, clock[0]
    assert " -- " not in clock[0], clock[0]


def test_behind_the_band_select_front_end_every_frame_is_whole(tmp_path):
    """61.44 MS/s ci8, one second, --decimate 6: the context runs at 10.24 MS/s, 1025/1024"""
    s = dict(fm.SCENE_61M44_D6, fmt=irdm.FMT_CI8, secs=1.0)
    x, expect, _ = fm.wideband_scene(s)
    wide = tmp_path / "wide.ci8"
    x.tofile(str(wide))
    del x
    centre = 1615000000.0
    r = run_cli(["-f", wide, "-r", s["fs_in"], "-c", "%.3f" % centre, "--band-center", "%.3f" % (centre + s["shift_hz"]),
                 "--decimate", s["D"], "--burst-resample", "--file-info", "fe", "--chunk", 1 << 20, "-v"], timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"burst resample: 249756.0976 -> 250000 samples/s per burst (1025/1024), 20 taps per phase\n" in r.stderr, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(expect) == s["n_inband"]
    # (whole by the rule of frontend_model.check_scene_demods for this scene: every bit of the unique word and the payload
    # right; the demodulator may follow the burst's tail for one symbol more)
    for l, e in zip(lines, expect):
        assert bits_of_line(l)[:len(e)] == e, l


def test_a_rate_whose_l_exceeds_4096_exits_2(rtl):
    r = run_cli(["-f", rtl["path"], "-r", 2_049_877, "--format", "cu8", "--burst-resample"])
    assert r.returncode == 2 and r.stdout == b"", (r.returncode, r.stderr.decode()[-500:])
    assert b"L = 2000000 is beyond 4096" in r.stderr


def test_on_the_grid_the_flag_changes_no_output(tmp_path):
    iq, _ = bc.scene(2_000_000)
    path = tmp_path / "grid.cf32"
    iq.tofile(str(path))
    args = ["-f", path, "-r", 2_000_000, "--file-info", "t", "--start-time", "1700000000"]
    a, b = run_cli(args), run_cli(args + ["--burst-resample"])
    assert a.returncode == b.returncode == 0
    assert a.stdout == b.stdout and a.stdout.count(b"RAW: ") >= 6
    strip = lambda e: [l for l in e.decode().splitlines() if not l.startswith("irdm timing:") and "Runtime" not in l]
    assert strip(a.stderr) == strip(b.stderr)
