"""The symbol clock check on the GPU (option symbol_clock, csrc/symbol_clock.hpp): the kernel against the float64 model of
tests/clock_model.py through irdm_symbol_clock_batch; the context option against the truth of scenes generated off the
250 kHz grid, at pipeline_depth 0 and 3, in one feed and in three; irdm_reset; the option set and cleared; --clock-check."""
import os
import re
import subprocess

import numpy as np
import pytest

import clock_checks as cc
import clock_model as cm
import irdm
import siggen

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
CLOCK_RE = re.compile(r"^clock: (\d+) frames; symbol clock ([-+]\d+\.\d\d) % \(quartiles ([-+]\d+\.\d\d) % \.\. ([-+]\d+\.\d\d) %\); "
                      r"(\d+) not ok, (\d+) out of range( -- the samples look like (\d+) S/s, not (\d+): check -r, or --resample-to (\d+))?$")


def scene(fs):
    return siggen.standard_scene(fs, fs // 2, 12, 3)[0]


@pytest.fixture(scope="module")
def stage():
    p = irdm.Pipeline(2_000_000, max_chunk_samples=32768 * 8, max_bursts_per_chunk=64, pipeline_depth=0)
    try:
        yield cc.stage_cases(p)
    finally:
        p.close()


def test_kernel_equals_the_model(stage):
    """irdm_symbol_clock_batch on the frames of clock_checks.kernel_frames (cut from the oracle's frames of the 10.025 MHz
    scene; lengths 63 / 64 / 65 / 1910 / 4440; all zero, NaN, Inf, noise; a line just beyond the grid edge) and in batches
    of 1, 63 and 65 frames over a context of 64 bursts per launch: flags and n equal the model's, |eps - eps_model| within
    4 x the largest value measured on the CPU emulation (clock_checks.EPS_TOL, 7.4e-9 against the 1e-4 allowed)"""
    assert stage["frames"] >= 5 + 9 + 6 and stage["worst"] <= cc.EPS_TOL


def test_frame_resampled_by_0_9_is_out_of_range(stage):
    """A frame resampled by 0.9 (tests/resample_model.py: 9.02 samples per symbol, eps -9.8 %) has its line 0.0022 cycles
    per sample, 3.9 widths of its main lobe, beyond the -8 % edge of the grid: the grid holds the frame's modulation alone
    (its maximum at +7.1 %, quality 5.2), the guard points beside the grid hold the line, twice as high -- out of range."""
    print("resampled by 0.9: flags %d eps %+.4f quality %.2f" % (stage["far_edge_flags"], stage["far_edge_eps"], stage["far_edge_quality"]))
    assert stage["far_edge_flags"] == cm.OUT_OF_RANGE


@pytest.mark.parametrize("fs", [10_000_000, 10_025_000, 10_050_000, 10_200_000, 2_400_000])
def test_truth(fs):
    """standard_scene(fs, fs // 2, 12, 3) through a context with the option on: the median within 0.05 % (absolute) of
    sps_scene / (10 decim) - 1 -- the float64 model alone stays within 0.027 % --, at least 5 frames used, the per-frame
    records byte for byte the same at pipeline_depth 0 and 3 and in one feed and three, the summary their histogram; and
    irdm_reset clears the summary"""
    iq = scene(fs)
    n = len(iq)
    seen = {}

    def reset_clears(p):
        p.poll_bursts(), p.poll_frames()
        p.reset(start_time_ns=1700000000 * 10**9)
        st = p.symbol_clock()
        assert (st.frames_used, st.frames_not_ok, st.frames_out_of_range, st.median, st.q25, st.q75) == (0, 0, 0, 0.0, 0.0, 0.0)
        assert p.poll_symbol_clock() == []
        seen["reset"] = True

    st0, c0, d0, _ = cc.context_run(iq, fs, [n], 0, after=reset_clears)
    rec = cc.check_summary(st0, c0)
    truth = cm.truth(fs)
    print("fs %d truth %+.4f %% median %+.4f %% quartiles %+.4f %% .. %+.4f %% used %d of %d" %
          (fs, 100 * truth, 100 * st0.median, 100 * st0.q25, 100 * st0.q75, st0.frames_used, len(rec)))
    assert seen["reset"]
    assert st0.frames_used >= 5
    assert abs(st0.median - truth) <= 5e-4, (st0.median, truth)
    decim = int(round(fs / 250000))
    assert st0.implied_rate_hz == 250000.0 * decim * (1.0 + st0.median)
    # the records without NOT_OK pair with the demodulator's records
    ids = np.frombuffer(d0.tobytes(), dtype=np.uint64).reshape(len(d0), -1)[:, 0]
    assert list(rec["id"][(rec["flags"] & cm.NOT_OK) == 0]) == list(ids)
    st1, c1, d1, _ = cc.context_run(iq, fs, [n], 3)
    st2, c2, d2, _ = cc.context_run(iq, fs, cc.ragged3(n), 0)
    assert c1.tobytes() == c0.tobytes() and c2.tobytes() == c0.tobytes()
    assert bytes(st1) == bytes(st0) and bytes(st2) == bytes(st0)
    assert d1.tobytes() == d0.tobytes() and d2.tobytes() == d0.tobytes()


def test_packed_records_carry_the_same_estimates():
    """the chain's packed record mode runs the kernel too: the same clock records as the full record mode"""
    fs = 10_025_000
    iq = scene(fs)
    _, c0, _, _ = cc.context_run(iq, fs, [len(iq)], 0)
    st, c1, d1, _ = cc.context_run(iq, fs, cc.ragged3(len(iq)), 3, packed=True)
    assert c1.tobytes() == c0.tobytes() and st.frames_used >= 5 and len(d1) == st.frames_used + st.frames_out_of_range


def test_option_off_changes_nothing():
    """a context that never had the option set and one that had it set to 1 and back to 0: the same demodulator records and
    counters, and no clock records on either; a member of a group refuses the option"""
    fs = 10_000_000
    iq = scene(fs)
    st_a, c_a, d_a, s_a = cc.context_run(iq, fs, [len(iq)], 0, options=())
    st_b, c_b, d_b, s_b = cc.context_run(iq, fs, [len(iq)], 0, options=(("symbol_clock", 1), ("symbol_clock", 0)))
    assert st_a is None and len(c_a) == 0 and len(c_b) == 0
    assert len(d_a) >= 5 and d_a.tobytes() == d_b.tobytes() and s_a == s_b
    cc.group_refuses()


def run_cli(args):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=180)


def test_cli(tmp_path):
    """the 10.025 MHz scene as cf32 read with -r 10000000: the clock line with the clause that names 10025000; the 10 MHz
    scene: the line without the clause; stdout and the other stderr lines those of the plain run; --gpus 2 and --save-only
    with the flag exit 2"""
    for fs, clause in ((10_025_000, True), (10_000_000, False)):
        path = tmp_path / ("s%d.cf32" % fs)
        scene(fs).tofile(path)
        common = ["-f", str(path), "-r", "10000000", "--start-time", "1700000000", "--file-info", "ck"]
        plain, check = run_cli(common), run_cli(common + ["--clock-check"])
        both = run_cli(common + ["--clock-check", "--input-stats"])
        assert plain.returncode == check.returncode == both.returncode == 0, (plain.stderr, check.stderr)
        assert check.stdout == plain.stdout == both.stdout and plain.stdout.count("RAW: ") >= 5
        pl, cl, bl = plain.stderr.splitlines(), check.stderr.splitlines(), both.stderr.splitlines()
        assert pl[-1].startswith("burst_detect: tagged ") and cl[:-1] == pl
        assert bl[:-2] == pl and bl[-2] == cl[-1] and bl[-1].startswith("input: ")
        g = CLOCK_RE.match(cl[-1])
        print(cl[-1])
        assert g, cl[-1]
        assert int(g.group(1)) >= 5 and abs(float(g.group(2)) / 100 - cm.truth(fs)) <= 5e-4 + 5e-5
        assert float(g.group(3)) <= float(g.group(2)) <= float(g.group(4))
        assert (g.group(7) is not None) == clause
        if clause:
            assert (g.group(8), g.group(9), g.group(10)) == ("10025000", "10000000", "10000000")
    r = run_cli(["-f", str(path), "-r", "10000000", "--clock-check", "--gpus", "2"])
    assert r.returncode == 2 and r.stdout == "" and "--clock-check" in r.stderr
    r = run_cli(["-f", str(path), "-r", "10000000", "--resample-to", "2500000", "--clock-check", "--save-band", str(tmp_path / "b.ci8"), "--save-only"])
    assert r.returncode == 2 and r.stdout == "" and "--clock-check" in r.stderr
    assert not (tmp_path / "b.ci8").exists()


def test_cli_too_few_frames(tmp_path):
    """a recording with fewer than 5 usable frames: no judgement"""
    fs = 2_000_000
    iq, _ = siggen.standard_scene(fs, 20 * 32768, 2, 7)
    path = tmp_path / "few.cf32"
    iq.tofile(path)
    r = run_cli(["-f", str(path), "-r", str(fs), "--clock-check"])
    assert r.returncode == 0, r.stderr
    assert re.match(r"^clock: [0-4] frames; too few to judge$", r.stderr.splitlines()[-1]), r.stderr
