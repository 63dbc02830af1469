"""--fine-freq of the command-line program: the RAW: lines carry the refined frequency, the closing "freq:" line stands
behind "clock:" and in front of "iq:", stdout without the flag is unchanged, and --gpus 2 / --save-only are refused."""
import os
import re
import subprocess

import numpy as np
import pytest

import fine_freq_checks as fc
import fine_freq_scenes as sc
import irdm

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
FS = 2_000_000
FREQ_RE = re.compile(r"^freq: (\d+) frames refined \((\d+) kept the PLL's value: (\d+) out of range, (\d+) invalid\); "
                     r"refined - PLL median ([-+]\d+) Hz \(quartiles ([-+]\d+) \.\. ([-+]\d+)\)$")


def run_cli(args):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=180)


def raw_fields(stdout):
    return [l.split() for l in stdout.splitlines() if l.startswith("RAW: ")]


def test_cli(tmp_path):
    iq, _ = sc.standard(FS, 3, 0.05)
    path = tmp_path / "s.cf32"
    np.asarray(iq).tofile(path)
    common = ["-f", str(path), "-r", str(FS), "--start-time", "1700000000", "--file-info", "ff"]
    plain, fine = run_cli(common), run_cli(common + ["--fine-freq"])
    assert plain.returncode == fine.returncode == 0, (plain.stderr, fine.stderr)
    # the library's records of the same stream
    on = fc.context_run(iq, FS, [len(iq)], 0)
    off = fc.context_run(iq, FS, [len(iq)], 0, options=())
    f_on, f_off = fc.frequencies(on["demods"]), fc.frequencies(off["demods"])
    a, b = raw_fields(plain.stdout), raw_fields(fine.stdout)
    assert len(a) == len(b) == len(f_on) >= 14
    # field 3 of a RAW: line is the frequency rounded to a whole Hz; every other field is that of the plain run
    assert [int(x[3]) for x in b] == [int(f + 0.5) for f in f_on]
    assert [int(x[3]) for x in a] == [int(f + 0.5) for f in f_off]
    assert [x[:3] + x[4:] for x in a] == [x[:3] + x[4:] for x in b]
    assert sum(x[3] != y[3] for x, y in zip(a, b)) >= 10
    # stderr: the plain run's lines and the closing line
    pl, fl = plain.stderr.splitlines(), fine.stderr.splitlines()
    assert pl[-1].startswith("burst_detect: tagged ") and fl[:-1] == pl
    g = FREQ_RE.match(fl[-1])
    print(fl[-1])
    assert g, fl[-1]
    st = on["summary"]
    assert (int(g.group(1)), int(g.group(3)), int(g.group(4))) == (st.frames_applied, st.frames_out_of_range, st.frames_invalid)
    assert int(g.group(2)) == st.frames_out_of_range + st.frames_invalid
    assert (float(g.group(5)), float(g.group(6)), float(g.group(7))) == (st.median, st.q25, st.q75)
    # its place: behind "clock:", in front of "iq:"; stdout does not depend on the other flags
    both = run_cli(common + ["--iq-check", "--fine-freq", "--clock-check", "-v"])
    assert both.returncode == 0 and both.stdout == fine.stdout
    bl = both.stderr.splitlines()
    i = [k for k, l in enumerate(bl) if l.startswith("freq: ")]
    assert len(i) == 1 and bl[i[0]] == fl[-1] and bl[i[0] - 1].startswith("clock: ") and bl[i[0] + 1].startswith("iq: ")
    assert sum(l.startswith("fine freq: ") for l in bl) == 1
    # without the flag nothing of it shows
    assert "freq:" not in plain.stderr and run_cli(common + ["--clock-check"]).stdout == plain.stdout


def test_cli_refusals(tmp_path):
    path = tmp_path / "n.cf32"
    np.zeros(65536, np.complex64).tofile(path)
    r = run_cli(["-f", str(path), "-r", str(FS), "--fine-freq", "--gpus", "2"])
    assert r.returncode == 2 and r.stdout == "" and "--fine-freq" in r.stderr
    r = run_cli(["-f", str(path), "-r", "10000000", "--resample-to", "2500000", "--fine-freq", "--save-band", str(tmp_path / "b.ci8"),
                 "--save-only"])
    assert r.returncode == 2 and r.stdout == "" and "--fine-freq" in r.stderr
    assert not (tmp_path / "b.ci8").exists()


def test_cli_no_frames(tmp_path):
    """a recording without a frame: "freq: 0 frames" """
    path = tmp_path / "n.cf32"
    rng = np.random.default_rng(1)
    (0.002 * (rng.standard_normal(1 << 21) + 1j * rng.standard_normal(1 << 21))).astype(np.complex64).tofile(path)
    r = run_cli(["-f", str(path), "-r", str(FS), "--fine-freq"])
    assert r.returncode == 0 and r.stdout == "" and r.stderr.splitlines()[-1] == "freq: 0 frames", r.stderr
