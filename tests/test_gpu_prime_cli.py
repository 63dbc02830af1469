"""The binary's --prime and --join on the GPU.  --prime: stdout is the lines formatted from the oracle's records over P || x
(tests/prime_checks.py), from a file, through standard input, from a WAV and for two recordings of a batch, and the closing
lines and side files are those of the run without the flag.  --join: a recording cut at arbitrary samples, as raw files and
as WAVs, prints the uncut run's stdout and stderr byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import containers as ct
import irdm
import parity
import prime_checks as pc

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
COMMON = ["-r", pc.FS, "--file-info", "t", "--start-time", "1700000000", "--chunk", pc.CHUNK]
CUTS = (1_000_001, 1_020_000)           # (the middle part, 19 999 samples, is smaller than a feed_block)
START = (2023, 11, 14, 22, 13, 20)      # 1700000000 s as a SYSTEMTIME, without the milliseconds


def run_cli(args, stdin=None):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, stdin=stdin, timeout=180)


def lines_equal(stdout, ref):
    """the binary's lines against the oracle's (orc_format_raw): the rule of tests/test_gpu_parity.py -- every field equal but
    the frequency (1 Hz) and the level (1e-4), whose last digit is soft -- and the time stamps equal too: the start time is given"""
    lines, want = stdout.decode().splitlines(), [l.strip() for l in ref.raw_lines("t")]
    assert len(lines) == len(want), (len(lines), len(want))
    for a, b in zip(lines, want):
        fa, fb = parity.raw_fields(a), parity.raw_fields(b)
        assert fa[:2] == fb[:2] and fa[3:6] == fb[3:6] and fa[7:] == fb[7:], (a, b)
        assert abs(fa[2] - fb[2]) <= 1 and abs(fa[6] - fb[6]) <= 1e-4, (a, b)
    return len(lines)


def parts_of(x):
    return [x[lo:hi] for lo, hi in zip((0,) + CUTS, CUTS + (len(x),))]


def float_wav(x, ms=None):
    """cf32 samples as a 32-bit float WAV at 2 MS/s; ms: with an auxi chunk that starts START + ms milliseconds"""
    aux = [ct.auxi_chunk(START + (ms,), START + (ms,), 1_622_000_000)] if ms is not None else []
    return ct.wav(np.ascontiguousarray(x).tobytes(), tag=ct.FLOAT, bits=32, rate=pc.FS, before=aux)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("prime")
    out = {"dir": d}
    for name in ("full", "excerpt"):
        x = pc.scene(name)[0]
        out[name] = d / (name + ".cf32")
        x.tofile(out[name])
    x = pc.scene("full")[0]
    out["wav"] = d / "full.wav"
    out["wav"].write_bytes(float_wav(x))
    for kind in ("raw", "wav", "late"):
        out[kind + "_parts"] = []
        for k, part in enumerate(parts_of(x)):
            path = d / ("part%d_%s.%s" % (k, kind, "cf32" if kind == "raw" else "wav"))
            if kind == "raw":
                part.tofile(path)
            else:
                # (the parts start 0, 500.0005 and 510 ms into the capture; the last one of "late" claims 515)
                ms = None if kind == "wav" else (0, 500, 515)[k]
                path.write_bytes(float_wav(part, ms))
            out[kind + "_parts"].append(path)
    return out


def join_args(paths):
    return [a for p in paths for a in ("-f", p)] + ["--join"]


# ---------------------------------------------------------------- --prime ----
def test_prime_prints_the_oracles_lines_over_the_prefixed_stream(files):
    """the 3 000 000-sample scene as a file, through standard input and as a WAV: 16 lines where the run without the flag
    prints 10; the excerpt shorter than the priming length: 6 lines for none; -v says what the prefix was made of"""
    ref = pc.scene("full")[1]
    plain = run_cli(["-f", files["full"]] + COMMON)
    assert plain.returncode == 0 and plain.stdout.count(b"RAW: ") == 10, plain.stderr
    a = run_cli(["-f", files["full"], "--prime", "-v"] + COMMON)
    assert a.returncode == 0 and lines_equal(a.stdout, ref) == 16, a.stderr
    assert a.stderr.decode().count("primed: 512 frames from the first 512\n") == 1
    assert b"tagged 16 bursts total" in a.stderr and b"primed:" not in plain.stderr
    with open(files["full"], "rb") as f:
        b = run_cli(["-f", "-", "--format", "cf32", "--prime"] + COMMON, stdin=f)
    assert b.returncode == 0 and b.stdout == a.stdout, b.stderr
    c = run_cli(["-f", files["wav"], "--prime"] + COMMON[2:])
    assert c.returncode == 0 and c.stdout == a.stdout, c.stderr
    e = run_cli(["-f", files["excerpt"], "--prime", "-v"] + COMMON)
    assert e.returncode == 0 and lines_equal(e.stdout, pc.scene("excerpt")[1]) == 6, e.stderr
    assert b"primed: 512 frames from the first 341\n" in e.stderr
    e0 = run_cli(["-f", files["excerpt"]] + COMMON)
    assert e0.returncode == 0 and e0.stdout == b"" and b"tagged 0 bursts total" in e0.stderr


def test_prime_in_a_batch_primes_every_recording(files):
    """two recordings in one run, each behind its reset: each prints what its own primed run prints"""
    (files["dir"] / "list.txt").write_text("%s 1700000000\n%s 1700000000\n" % (files["excerpt"], files["full"]))
    r = run_cli(["--files-from", files["dir"] / "list.txt", "--prime", "--out-dir", files["dir"] / "out"] + COMMON)
    assert r.returncode == 0, r.stderr
    assert lines_equal((files["dir"] / "out" / "excerpt.cf32.out").read_bytes(), pc.scene("excerpt")[1]) == 6
    assert lines_equal((files["dir"] / "out" / "full.cf32.out").read_bytes(), pc.scene("full")[1]) == 16
    assert [l for l in r.stderr.decode().splitlines() if "tagged" in l] == ["burst_detect: tagged 6 bursts total", "burst_detect: tagged 16 bursts total"]


def test_closing_lines_and_the_spectrum_file_are_those_of_the_unprimed_run(files):
    """--input-stats --scrub --image-check and --spectrum with and without --prime: the input:, scrub: and image: lines agree
    but for the image line's count of frames (there are more of them), and the spectrum file is the same bytes"""
    spec = [files["dir"] / "plain.spec", files["dir"] / "primed.spec"]
    flags = ["--input-stats", "--scrub", "--image-check", "--spectrum-frames", 100]
    a = run_cli(["-f", files["full"], "--spectrum", spec[0]] + flags + COMMON)
    b = run_cli(["-f", files["full"], "--spectrum", spec[1], "--prime"] + flags + COMMON)
    assert a.returncode == b.returncode == 0, (a.stderr, b.stderr)
    la, lb = a.stderr.decode().splitlines(), b.stderr.decode().splitlines()
    print(lb)
    assert len(la) == len(lb) == 4 and la[0] == "burst_detect: tagged 10 bursts total" and lb[0] == "burst_detect: tagged 16 bursts total"
    assert la[1].startswith("image: 3000000 samples;") and la[1].replace("of 10 frames", "of 16 frames") == lb[1]
    assert la[2] == lb[2] == "scrub: 3000000 samples cf32, limit 2^40; none zeroed"
    assert la[3] == lb[3] and la[3].startswith("input: 3000000 samples cf32;")
    assert spec[0].stat().st_size > 64 + 14 * (32 + 8 * 2048) and spec[0].read_bytes() == spec[1].read_bytes()


def test_save_band_behind_the_front_end_is_the_unprimed_runs_file(files):
    """--prime behind --resample-to (the file read as a 2.4 MS/s capture, 5/6): the saved band is the unprimed run's file,
    byte for byte, and the primed run ends no poorer in lines"""
    band = [files["dir"] / "plain.band.cf32", files["dir"] / "primed.band.cf32"]
    args = ["-r", "2400000", "--resample-to", "2000000", "--file-info", "t", "--start-time", "1700000000"]
    a = run_cli(["-f", files["full"], "--save-band", band[0]] + args)
    b = run_cli(["-f", files["full"], "--save-band", band[1], "--prime", "-v"] + args)
    assert a.returncode == b.returncode == 0, (a.stderr, b.stderr)
    assert band[0].stat().st_size > 8 * 2_000_000 and band[0].read_bytes() == band[1].read_bytes()
    assert b"primed: 512 frames from the first 512\n" in b.stderr
    assert b.stdout.count(b"RAW: ") >= a.stdout.count(b"RAW: ")


def test_prime_refusals_and_a_recording_shorter_than_a_frame(files):
    """--prime with --save-only and with --gpus 2 exit with 2; a recording shorter than one FFT frame runs unprimed with one
    warning"""
    for extra in (["--gpus", "2"], ["--resample-to", "1000000", "--save-band", files["dir"] / "x.cf32", "--save-only"]):
        r = run_cli(["-f", files["full"], "--prime"] + extra + COMMON)
        assert r.returncode == 2 and r.stdout == b"" and b"--prime" in r.stderr, (extra, r.stderr)
    tiny = files["dir"] / "tiny.cf32"
    pc.scene("full")[0][:2047].tofile(tiny)
    r = run_cli(["-f", tiny, "--prime"] + COMMON)
    assert r.returncode == 0 and r.stderr.decode().count("warning: --prime:") == 1 and b"runs unprimed" in r.stderr, r.stderr


# ---------------------------------------------------------------- --join ----
def test_join_prints_the_uncut_runs_output(files):
    """the scene cut at samples 1 000 001 and 1 020 000, as three raw files and as three WAVs, --chunk 262144: stdout and stderr
    of the uncut run, byte for byte; --prime --join equals --prime over the uncut file"""
    whole = run_cli(["-f", files["full"]] + COMMON)
    assert whole.returncode == 0 and whole.stdout.count(b"RAW: ") == 10
    raw = run_cli(join_args(files["raw_parts"]) + COMMON)
    assert raw.returncode == 0 and (raw.stdout, raw.stderr) == (whole.stdout, whole.stderr), raw.stderr
    wav = run_cli(join_args(files["wav_parts"]) + COMMON[2:])
    assert wav.returncode == 0 and (wav.stdout, wav.stderr) == (whole.stdout, whole.stderr), wav.stderr
    primed = run_cli(["-f", files["full"], "--prime"] + COMMON)
    both = run_cli(join_args(files["raw_parts"]) + ["--prime"] + COMMON)
    assert both.returncode == 0 and (both.stdout, both.stderr) == (primed.stdout, primed.stderr) and primed.stdout.count(b"RAW: ") == 16
    listed = files["dir"] / "parts.txt"
    listed.write_text("".join("%s\n" % p for p in files["raw_parts"][1:]))
    mixed = run_cli(["-f", files["raw_parts"][0], "--files-from", listed, "--join"] + COMMON)
    assert (mixed.stdout, mixed.stderr) == (whole.stdout, whole.stderr)


def test_join_warns_about_a_part_whose_header_time_is_off(files):
    """three WAVs with auxi times 0, 500 and 515 ms: the third part starts at 510 ms of the stream, 5 ms early for its header
    -- one warning that names it; the second part's half microsecond draws none; nothing else changes"""
    whole = run_cli(["-f", files["full"]] + COMMON)
    r = run_cli(join_args(files["late_parts"]) + ["--file-info", "t", "--chunk", pc.CHUNK])
    assert r.returncode == 0 and r.stdout == whole.stdout, r.stderr
    err = r.stderr.decode().splitlines()
    warn = [l for l in err if l.startswith("warning: --join:")]
    assert len(warn) == 1 and str(files["late_parts"][2]) in warn[0] and "0.005000 s later" in warn[0], err
    assert [l for l in err if l not in warn] == whole.stderr.decode().splitlines()


def test_join_refusals(files):
    """mixed formats, mixed rates, -f - beside another file and --gpus 2: exit 2 before anything runs"""
    x = pc.scene("full")[0][:65536]
    ci16 = files["dir"] / "other.ci16"
    np.zeros(2 * 65536, np.int16).tofile(ci16)
    slow = files["dir"] / "slow.wav"
    slow.write_bytes(ct.wav(np.ascontiguousarray(x).tobytes(), tag=ct.FLOAT, bits=32, rate=1_000_000))
    for args in (["-f", files["raw_parts"][0], "-f", ci16, "--join"] + COMMON,
                 ["-f", files["wav_parts"][0], "-f", slow, "--join"] + COMMON[2:],
                 ["-f", files["wav_parts"][0], "-f", slow, "--join"] + COMMON,
                 ["-f", files["raw_parts"][0], "-f", "-", "--join"] + COMMON,
                 join_args(files["raw_parts"]) + ["--gpus", "2"] + COMMON):
        r = run_cli(args, stdin=subprocess.DEVNULL)
        assert r.returncode == 2 and r.stdout == b"", (args, r.stderr)
