"""--fine-time of the command-line program: the RAW: lines carry the refined time and differ from the plain run's in the time
field only, the closing "time:" line stands behind "freq:" and in front of "iq:", a rate off the 250 kHz grid is warned of
once unless --burst-resample is given, and --gpus 2 / --save-only are refused."""
import os
import re
import subprocess

import numpy as np
import pytest

import fine_freq_scenes as sc
import fine_time_checks as fc
import irdm

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
FS = 2_000_000
TIME_RE = re.compile(r"^time: (\d+) frames refined \((\d+) kept the correlator's place: (\d+) ambiguous, (\d+) invalid\); "
                     r"line - correlator median ([-+]\d+\.\d\d) samples \(quartiles ([-+]\d+\.\d\d) \.\. ([-+]\d+\.\d\d)\)$")


def run_cli(args):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=180)


def raw_fields(stdout):
    return [l.split() for l in stdout.splitlines() if l.startswith("RAW: ")]


def test_cli(tmp_path):
    iq, _ = sc.standard(FS, 3, 0.05)
    path = tmp_path / "s.cf32"
    np.asarray(iq).tofile(path)
    common = ["-f", str(path), "-r", str(FS), "--start-time", "1700000000", "--file-info", "ft"]
    plain, fine = run_cli(common), run_cli(common + ["--fine-time"])
    assert plain.returncode == fine.returncode == 0, (plain.stderr, fine.stderr)
    # the library's records of the same stream
    on = fc.context_run(iq, FS, [len(iq)], 0, packed=True)
    off = fc.context_run(iq, FS, [len(iq)], 0, options=(), packed=True)
    t_on, t_off = fc.times(on["demods"]), fc.times(off["demods"])
    a, b = raw_fields(plain.stdout), raw_fields(fine.stdout)
    assert len(a) == len(b) == len(t_on) >= 14
    # field 2 of a RAW: line is the time in ms behind the whole second of the first frame, to 0.1 us; every other field is
    # that of the plain run
    t0 = sc.START_NS
    assert [x[2] for x in b] == ["%012.4f" % ((int(t) - t0) / 1e6) for t in t_on]
    assert [x[2] for x in a] == ["%012.4f" % ((int(t) - t0) / 1e6) for t in t_off]
    assert [x[:2] + x[3:] for x in a] == [x[:2] + x[3:] for x in b]
    # about 0.73 ms later: the correlator's peak is near sample 189 of 250 kHz
    d = np.array([float(y[2]) - float(x[2]) for x, y in zip(a, b)])
    assert np.all(d > 0.65) and np.all(d < 0.80), d
    # stderr: the plain run's lines and the closing line
    pl, fl = plain.stderr.splitlines(), fine.stderr.splitlines()
    assert pl[-1].startswith("burst_detect: tagged ") and fl[:-1] == pl
    g = TIME_RE.match(fl[-1])
    print(fl[-1])
    assert g, fl[-1]
    st = on["summary"]
    assert (int(g.group(1)), int(g.group(3)), int(g.group(4))) == (st.frames_applied, st.frames_ambiguous, st.frames_invalid)
    assert int(g.group(1)) == len(b) and int(g.group(2)) == st.frames_ambiguous + st.frames_invalid == 0
    assert (g.group(5), g.group(6), g.group(7)) == ("%+.2f" % st.median, "%+.2f" % st.q25, "%+.2f" % st.q75)
    # its place: behind "freq:", in front of "iq:"; with --fine-freq beside it the lines differ from fine's in the frequency alone
    both = run_cli(common + ["--iq-check", "--fine-time", "--fine-freq", "--clock-check", "-v"])
    assert both.returncode == 0
    c = raw_fields(both.stdout)
    assert [x[:3] + x[4:] for x in c] == [x[:3] + x[4:] for x in b]
    bl = both.stderr.splitlines()
    i = [k for k, l in enumerate(bl) if l.startswith("time: ")]
    assert len(i) == 1 and bl[i[0]] == fl[-1] and bl[i[0] - 1].startswith("freq: ") and bl[i[0] + 1].startswith("iq: ")
    assert sum(l.startswith("fine time: ") for l in bl) == 1
    # without the flag nothing of it shows; at a rate on the grid there is no warning
    assert "time:" not in plain.stderr and "warning" not in fine.stderr


def test_cli_warns_off_the_grid(tmp_path):
    """2.4 MS/s is 240 kHz per burst: one warning that names --burst-resample, none with that flag, none without --fine-time"""
    path = tmp_path / "n.cf32"
    rng = np.random.default_rng(1)
    (0.002 * (rng.standard_normal(1 << 21) + 1j * rng.standard_normal(1 << 21))).astype(np.complex64).tofile(path)
    common = ["-f", str(path), "-r", "2400000"]
    r = run_cli(common + ["--fine-time"])
    assert r.returncode == 0 and r.stderr.splitlines()[-1] == "time: 0 frames", r.stderr
    w = [l for l in r.stderr.splitlines() if "--fine-time" in l]
    assert len(w) == 1 and w[0].startswith("warning: ") and "--burst-resample" in w[0] and "2400000" in w[0], r.stderr
    r = run_cli(common + ["--fine-time", "--burst-resample"])
    assert r.returncode == 0 and "--fine-time" not in r.stderr and "warning" not in r.stderr, r.stderr
    assert r.stderr.splitlines()[-1] == "time: 0 frames"
    r = run_cli(common + ["--burst-resample"])
    assert r.returncode == 0 and "time:" not in r.stderr and "--fine-time" not in r.stderr


def test_cli_refusals(tmp_path):
    path = tmp_path / "n.cf32"
    np.zeros(65536, np.complex64).tofile(path)
    r = run_cli(["-f", str(path), "-r", str(FS), "--fine-time", "--gpus", "2"])
    assert r.returncode == 2 and r.stdout == "" and "--fine-time" in r.stderr
    r = run_cli(["-f", str(path), "-r", "10000000", "--resample-to", "2500000", "--fine-time", "--save-band", str(tmp_path / "b.ci8"),
                 "--save-only"])
    assert r.returncode == 2 and r.stdout == "" and "--fine-time" in r.stderr
    assert not (tmp_path / "b.ci8").exists()
