"""Self-describing recordings through the command line on the GPU: one 2 MHz scene written as raw cf32, as WAV (16-bit PCM
with an auxi chunk, 32-bit float), as SigMF ci16_le and as an .sdriq file at sample size 24.  A container run with -f alone
prints, byte for byte, what the raw file of the same samples prints when -r, -c, --start-time and --format are given by hand;
and --save-band x.sigmf-data writes a pair that reads back with -f alone."""
import os
import subprocess

import numpy as np
import pytest

import ci32
import containers as ct
import formats16 as f16
import frontend_model as fm
import irdm
import siggen

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
FS = 2_000_000
CENTRE = 1_626_000_000
START = (2023, 11, 14, 22, 13, 20, 250)
STOP = (2023, 11, 14, 22, 13, 21, 450)
START_ARG = "1700000000.250"


def run_exe(args, **kw):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """the scene in every form, and the stdout of the raw runs described by hand"""
    d = tmp_path_factory.mktemp("containers")
    n = int(1.2 * FS) // 32768 * 32768
    iq, _ = siggen.standard_scene(FS, n, 6, seed=162)
    i16 = siggen.to_ci16(iq, 131072.0)
    i24 = ci32.to_ci32(iq, irdm.FMT_CI32_24)
    x32 = (ct.interleave(iq) * np.float32(4.0)).astype(np.float32)
    aux = ct.auxi_chunk(START, STOP, CENTRE)
    files = {}

    def put(name, data):
        p = d / name
        p.write_bytes(data if isinstance(data, bytes) else data.encode())
        files[name] = p
        return p

    put("pcm16.wav", ct.wav(i16.tobytes(), rate=FS, bits=16, before=[aux]))
    put("pcm16_list.wav", ct.wav(i16.tobytes(), rate=FS, bits=16, before=[aux],
                                 after=[ct.chunk(b"LIST", np.full(200000, 32767, np.int16).tobytes())]))
    put("float32.wav", ct.wav(x32.tobytes(), tag=ct.FLOAT, rate=FS, bits=32, fmt_size=18, before=[aux]))
    put("SDRuno_20231114_221320Z_1626000kHz.wav", ct.wav(i16.tobytes(), rate=FS, bits=16))
    put("rec.sigmf-data", i16.tobytes())
    put("rec.sigmf-meta", ct.sigmf_meta("ci16_le", FS, frequency=CENTRE, datetime="2023-11-14T22:13:20.250Z"))
    put("rec.sdriq", ct.sdriq_header(FS, CENTRE, 1_700_000_000_250, 24) + i24.tobytes())
    put("raw16.bin", i16.tobytes())
    put("raw24.bin", i24.tobytes())
    put("raw32.cf32", x32.tobytes())
    put("conv16.cf32", f16.converted(i16, irdm.FMT_CI16_FULL).tobytes())
    put("conv24.cf32", ci32.converted(i24, irdm.FMT_CI32_24).tobytes())
    by_hand = ["-r", FS, "-c", CENTRE, "--start-time", START_ARG]
    want = {}
    for key, name, fmt in (("16", "raw16.bin", "ci16-full"), ("24", "raw24.bin", "ci32-24"), ("32", "raw32.cf32", "cf32"),
                           ("conv16", "conv16.cf32", "cf32"), ("conv24", "conv24.cf32", "cf32")):
        r = run_exe(["-f", files[name], "--format", fmt] + by_hand)
        assert r.returncode == 0 and r.stdout.count(b"RAW: ") >= 3, r.stderr.decode()[-2000:]
        want[key] = r.stdout
    # the integer files print what the cf32 files of their converted samples print
    assert want["16"] == want["conv16"] and want["24"] == want["conv24"]
    return dict(dir=d, files=files, want=want, by_hand=by_hand)


@pytest.mark.parametrize("name,key", [("pcm16.wav", "16"), ("float32.wav", "32"), ("rec.sigmf-meta", "16"), ("rec.sigmf-data", "16"),
                                      ("rec.sdriq", "24"), ("pcm16_list.wav", "16")])
def test_container_alone_prints_the_raw_runs_lines(forms, name, key):
    """-f FILE and nothing else; a trailing LIST chunk full of large values changes nothing"""
    r = run_exe(["-f", forms["files"][name]])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == forms["want"][key]
    assert b"warning" not in r.stderr


def test_flags_beside_a_header(forms):
    """a header without a time or a centre of its own takes them from the flags and the file's name; an explicit -c wins
    without a warning, an explicit -r that disagrees wins with one; --container reads a file of any name"""
    f = forms["files"]
    r = run_exe(["-f", f["SDRuno_20231114_221320Z_1626000kHz.wav"], "--start-time", START_ARG])
    assert r.returncode == 0 and r.stdout == forms["want"]["16"], r.stderr.decode()[-2000:]
    other = run_exe(["-f", f["raw16.bin"], "--format", "ci16-full", "-r", FS, "-c", CENTRE + 500_000, "--start-time", "1700000100"])
    r = run_exe(["-f", f["pcm16.wav"], "-c", CENTRE + 500_000, "--start-time", "1700000100"])
    assert r.returncode == 0 and r.stdout == other.stdout and r.stdout != forms["want"]["16"] and b"warning" not in r.stderr
    r = run_exe(["-f", f["pcm16.wav"], "-r", FS])
    assert r.returncode == 0 and r.stdout == forms["want"]["16"] and b"warning" not in r.stderr
    renamed = forms["dir"] / "renamed.bin"
    renamed.write_bytes(f["rec.sdriq"].read_bytes())
    r = run_exe(["-f", renamed, "--container", "sdriq", "-v"])
    assert r.returncode == 0 and r.stdout == forms["want"]["24"]
    assert ("probe: %s container=sdriq format=ci32-24 rate=2000000 centre=1626000000 start=1700000000.250000000 offset=32" % renamed).encode() in r.stderr


def test_rate_mismatch_warns_and_off_grid_rate_warns(tmp_path):
    """-r 4000000 beside a 2 MS/s header: the flag wins, one warning line; a 2.4 MS/s container without --resample-to: one
    warning that names the rate and the flag; a raw file at that rate: none"""
    noise = (np.random.default_rng(3).standard_normal(2 * 32768 * 8) * 300).astype(np.int16)
    w = tmp_path / "a.wav"
    w.write_bytes(ct.wav(noise.tobytes(), rate=2_000_000))
    r = run_exe(["-f", w, "-r", 4000000], text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [l for l in r.stderr.splitlines() if l.startswith("warning: ")] == \
        ["warning: %s: -r 4000000 overrides the header's 2000000 samples/s" % w]
    w24 = tmp_path / "b.wav"
    w24.write_bytes(ct.wav(noise.tobytes(), rate=2_400_000))
    r = run_exe(["-f", w24], text=True)
    warn = [l for l in r.stderr.splitlines() if l.startswith("warning: ")]
    assert r.returncode == 0 and len(warn) == 1 and "2400000" in warn[0] and "--resample-to" in warn[0], r.stderr[-2000:]
    r = run_exe(["-f", w24, "--resample-to", 2500000], text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-2000:]
    raw = tmp_path / "b.cs16"
    noise.tofile(raw)
    r = run_exe(["-f", raw, "-r", 2400000, "--format", "ci16-full"], text=True)
    assert r.returncode == 0 and "warning" not in r.stderr
    # ... nor beside a malformed container, which fails alone: the rate is -r's, no container gave it
    bad = tmp_path / "bad.sdriq"
    bad.write_bytes(b"\0" * 4096)
    r = run_exe(["-f", raw, "-f", bad, "-r", 2400000], text=True)
    assert r.returncode == 1 and "CRC-32" in r.stderr and "warning" not in r.stderr, r.stderr[-2000:]


def test_two_containers_in_one_run(forms, tmp_path):
    """different centres and start times in one run: what the two separate runs print, one after the other; a malformed one
    among them fails alone (exit 1)"""
    f = forms["files"]
    second = tmp_path / "second.sigmf-data"
    second.write_bytes(f["raw16.bin"].read_bytes())
    (tmp_path / "second.sigmf-meta").write_text(ct.sigmf_meta("ci16_le", FS, frequency=CENTRE + 1_000_000, datetime="2023-11-14T23:00:00.5Z"))
    a, b = run_exe(["-f", f["pcm16.wav"]]), run_exe(["-f", second])
    assert a.returncode == 0 and b.returncode == 0 and a.stdout != b.stdout
    both = run_exe(["-f", f["pcm16.wav"], "-f", second])
    assert both.returncode == 0 and both.stdout == a.stdout + b.stdout, both.stderr.decode()[-2000:]
    bad = tmp_path / "bad.sdriq"
    bad.write_bytes(b"\0" * 4096)
    three = run_exe(["-f", f["pcm16.wav"], "-f", bad, "-f", second])
    assert three.returncode == 1 and three.stdout == a.stdout + b.stdout and b"CRC-32" in three.stderr


def test_save_band_as_sigmf_reads_back_alone(tmp_path):
    """--save-band x.sigmf-data behind --decimate writes the band and x.sigmf-meta; -f x.sigmf-data alone then prints the
    stdout of the wideband run (the scene and arguments of tests/test_gpu_saveband.py)"""
    x, _, _ = fm.wideband_scene()
    s = fm.SCENE
    wide = tmp_path / "wide.ci8"
    x.tofile(str(wide))
    centre = 1615000000.0
    out = tmp_path / "x.sigmf-data"
    common = ["-f", wide, "-r", s["fs_in"], "-c", "%.3f" % centre, "--band-center", "%.3f" % (centre + s["shift_hz"]),
              "--decimate", s["D"], "--file-info", "fe", "--start-time", "1700000000", "--chunk", 1 << 20]
    base = run_exe(common)
    a = run_exe(common + ["--save-band", out])
    assert a.returncode == 0 and a.stdout == base.stdout and a.stdout.count(b"RAW: ") == s["n_inband"], a.stderr.decode()[-2000:]
    rc, info, msg = irdm.recording_probe(out)
    assert rc == 0 and info.format == irdm.FMT_CF32 and info.sample_rate == s["fs_in"] // s["D"], msg
    assert info.has_start and info.start_time_ns == 1700000000 * 10 ** 9 and info.has_center
    b = run_exe(["-f", out, "--file-info", "fe", "--chunk", 1 << 20])
    assert b.returncode == 0 and b.stdout == base.stdout, b.stderr.decode()[-2000:]
    out16 = tmp_path / "y.sigmf-data"
    c = run_exe(common + ["--save-band", out16, "--save-format", "ci16", "--save-gain", 4])
    assert c.returncode == 0 and irdm.recording_probe(out16)[1].format == irdm.FMT_CI16_FULL
    d = run_exe(["-f", tmp_path / "y.sigmf-meta", "--file-info", "fe", "--chunk", 1 << 20])
    assert d.returncode == 0 and d.stdout.count(b"RAW: ") == s["n_inband"]
