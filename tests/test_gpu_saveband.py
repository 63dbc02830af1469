"""Saving the band on the GPU (csrc/frontend.hip requant_kernel, csrc/frontend.cpp irdm_frontend_save): the requantiser
against the numpy model (tests/saveband_model.py) byte for byte, the recording behind the stage-level entries and the
feeder against the model applied to the front end model's output, with the pipeline's records unchanged, and the command
line (--save-band, --save-format, --save-gain, --save-only)."""
import os
import re
import subprocess

import numpy as np
import pytest

import frontend_model as fm
import irdm
import orc
import parity
import resample_model as rm
import saveband_model as sm

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
CASES = ((irdm.FMT_CI8, 2.0), (irdm.FMT_CI16, 0.37), (irdm.FMT_CF32, 1.0))
N_STAGE = (1 << 22) + 12345


def test_requantiser_equals_the_numpy_model():
    """irdm_requantize_device: the emulated test's sizes and 2^20 + 7, both formats, three gains, nine offset pairs"""
    sizes = sm.KERNEL_SIZES + ((1 << 20) + 7,)
    assert sm.check_kernel(sizes) == 2 * len(sm.GAINS) * len(sizes) * len(sm.OFFSETS) ** 2


@pytest.fixture(scope="module")
def stage_refs():
    """the captures of the stage cases and the models' outputs on them, computed once"""
    refs = {}
    fs_in, D, q = 4_000_000, 2, 14418
    taps = fm.design_taps(fs_in, D)
    for fmt in (irdm.FMT_CI8, irdm.FMT_CF32):
        x = fm.random_capture(fmt, N_STAGE, seed=40 + fmt)
        refs[fm.NAMES[fmt]] = (x, fm.run(x, fmt, D, q, taps), len(taps))
    fi, fo = 11_200_000, 10_000_000
    x = fm.random_capture(irdm.FMT_CI8, N_STAGE, seed=28)
    ptaps = rm.design_taps(fi, fo)
    refs["25/28"] = (x, rm.run(x, irdm.FMT_CI8, 25, 28, fm.quantise(150e3, fi), ptaps), len(ptaps))
    return refs


@pytest.mark.parametrize("slot", [4099, 0])
@pytest.mark.parametrize("name", ["ci8", "cf32", "25/28"])
def test_saved_band_equals_the_model_through_the_stage_entries(stage_refs, name, slot):
    """2^22 + 12345 input samples, whole and in ragged feeds, pieces of 4099 samples and of the default size: ci8 / ci16
    recordings = the numpy model on the front end model's output (K0 at D = 2, K0r at 25 / 28), cf32 = its bytes"""
    x, want_y, ntaps = stage_refs[name]
    if name == "25/28":
        fi, fo = 11_200_000, 10_000_000
        sh = fm.quantise(150e3, fi) * fi / 65536.0
        make = lambda: rm.Stage(fi, irdm.FMT_CI8, fo, sh)                              # noqa: E731
        feeds = [[N_STAGE], rm.ragged_feeds(N_STAGE, ntaps, 25, (99991,))]
    else:
        fmt = irdm.FMT_CI8 if name == "ci8" else irdm.FMT_CF32
        make = lambda: fm.Stage(4_000_000, fmt, 2, 14418 * 4_000_000 / 65536.0)        # noqa: E731
        feeds = [[N_STAGE], fm.ragged_feeds(N_STAGE, ntaps, (99991,))]
    assert sm.check_saved(make, x, want_y, feeds, CASES, slot) == 6


@pytest.fixture(scope="module")
def scene():
    """the wideband scene of tests/test_gpu_frontend.py, the model's output and the oracle's records on it"""
    x, expect, q = fm.wideband_scene()
    s = fm.SCENE
    taps = fm.design_taps(s["fs_in"], s["D"])
    applied = q * s["fs_in"] / 65536.0
    y = fm.run(x, irdm.FMT_CI8, s["D"], q, taps)
    ref = orc.run_stream(y, s["fs_in"] // s["D"], center_frequency=1622000000.0 + applied)
    return dict(x=x, expect=expect, q=q, y=y, ref=ref, applied=applied)


@pytest.mark.parametrize("depth,feed", [(0, "host"), (3, "host"), (0, "device"), (3, "device")])
def test_feeder_saves_the_band_and_the_pipeline_still_equals_the_oracle(scene, depth, feed):
    """irdm_frontend_feed_* + flush with saving on (ci16, gain 1) in front of a cf32 context, chunk 2^20: the sink's bytes are
    the model's, and the records pass parity.compare against the oracle on the model's output as they do with saving off"""
    s = fm.SCENE
    chunk = 1 << 20
    n = len(scene["x"]) // 2
    feeds = fm.block_feeds(n, s["D"] * chunk) if feed == "host" else fm.block_feeds(n, s["D"] * chunk - 12347)
    got, applied, saved, stats = sm.run_composed_saved(scene["x"], s["fs_in"], irdm.FMT_CI8, s["D"], s["shift_hz"], feeds, depth,
                                                       chunk, feed, irdm.FMT_CI16)
    want, wstats = sm.quantise(scene["y"], irdm.FMT_CI16, 1.0)
    assert applied == scene["applied"]
    assert saved == want, sm.first_difference(saved, want, irdm.FMT_CI16)
    assert sm.same_stats(stats, wstats) and wstats[1] == 0
    assert got["n_samples"] == len(scene["y"])
    summary = parity.compare(got, scene["ref"])
    assert summary["demods"] == s["n_inband"], summary
    fm.check_scene_demods(got["demods"], scene["expect"])


# ---- the command line ----
CAPTURE_CENTER = 1615000000.0


def run_exe(args, **kw):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, timeout=600, **kw)


@pytest.fixture(scope="module")
def cli(scene, tmp_path_factory):
    """the scene as a file, the common arguments of its runs, and the run without --save-band"""
    s = fm.SCENE
    d = tmp_path_factory.mktemp("saveband")
    wide = d / "wide.ci8"
    scene["x"].tofile(str(wide))
    common = ["-f", wide, "-r", s["fs_in"], "-c", "%.3f" % CAPTURE_CENTER, "--band-center", "%.3f" % (CAPTURE_CENTER + s["shift_hz"]),
              "--decimate", s["D"], "--file-info", "fe", "--start-time", "1700000000"]
    base = run_exe(common + ["--chunk", 1 << 20])
    assert base.returncode == 0 and base.stdout.count(b"RAW: ") == s["n_inband"], base.stderr.decode()[-2000:]
    narrow = ["-r", s["fs_in"] // s["D"], "-c", "%.17g" % (CAPTURE_CENTER + scene["applied"]), "--file-info", "fe",
              "--start-time", "1700000000", "--chunk", 1 << 20]
    return dict(dir=d, wide=wide, common=common, base=base, narrow=narrow)


def bit_fields(stdout):
    return [l.split()[-1] for l in stdout.decode().splitlines() if l.startswith("RAW: ")]


def test_cli_cf32_band_is_the_models_and_reads_back_to_the_same_lines(scene, cli):
    """--save-band out.cf32: the model's bytes; stdout and stderr those of the run without the flag; the binary on out.cf32 at
    the band's rate and centre prints the same stdout again"""
    out = cli["dir"] / "out.cf32"
    a = run_exe(cli["common"] + ["--chunk", 1 << 20, "--save-band", out])
    assert a.returncode == 0, a.stderr.decode()[-2000:]
    assert a.stdout == cli["base"].stdout and a.stderr == cli["base"].stderr
    assert out.read_bytes() == scene["y"].tobytes()
    b = run_exe(["-f", out] + cli["narrow"])
    assert b.returncode == 0 and b.stdout == cli["base"].stdout, b.stderr.decode()[-2000:]


@pytest.mark.parametrize("name,fmt,gain,read_as", [("out.ci8", irdm.FMT_CI8, 4.0, "ci8"), ("out.ci16", irdm.FMT_CI16, 1.0, "ci16-full")])
def test_cli_integer_bands_are_the_models_and_decode(scene, cli, name, fmt, gain, read_as):
    """--save-band out.ci8 --save-gain 4 and out.ci16: the numpy model's bytes, nothing clipped; read back with --format ci8 /
    ci16-full, six RAW lines whose bit fields are the wideband run's"""
    out = cli["dir"] / name
    a = run_exe(cli["common"] + ["--chunk", 1 << 20, "--save-band", out] + (["--save-gain", gain] if gain != 1.0 else []))
    assert a.returncode == 0, a.stderr.decode()[-2000:]
    assert a.stdout == cli["base"].stdout and a.stderr == cli["base"].stderr        # (no warning: nothing clips)
    want, wstats = sm.quantise(scene["y"], fmt, gain)
    assert wstats[1] == 0
    assert out.read_bytes() == want
    b = run_exe(["-f", out, "--format", read_as] + cli["narrow"])
    assert b.returncode == 0, b.stderr.decode()[-2000:]
    assert len(bit_fields(b.stdout)) == fm.SCENE["n_inband"] and bit_fields(b.stdout) == bit_fields(cli["base"].stdout)


def test_cli_clipping_is_counted_and_warned_of(scene, cli):
    """--save-gain 64 into ci8: a warning without -v; with -v the closing line, whose counts are the numpy model's"""
    out = cli["dir"] / "loud.ci8"
    want, wstats = sm.quantise(scene["y"], irdm.FMT_CI8, 64.0)
    assert wstats[1] > 0
    a = run_exe(cli["common"] + ["--chunk", 1 << 20, "--save-band", out, "--save-gain", 64])
    assert a.returncode == 0 and a.stdout == cli["base"].stdout
    extra = a.stderr.decode().replace(cli["base"].stderr.decode(), "")
    assert "--save-band: %s: %d of %d components clipped at gain 64" % (cli["wide"], wstats[1], 2 * wstats[0]) in extra, a.stderr
    assert out.read_bytes() == want
    v = run_exe(cli["common"] + ["--chunk", 1 << 20, "--save-band", out, "--save-gain", 64, "-v"])
    assert v.returncode == 0 and v.stdout == cli["base"].stdout
    m = re.search(r"saved band: (\d+) samples ci8 gain 64, peak ([0-9.]+) of full scale, (\d+) components clipped; "
                  r"read with -r 10000000 -c (\S+) --format ci8\n$", v.stderr.decode())
    assert m, v.stderr.decode()[-1000:]
    assert (int(m.group(1)), int(m.group(3))) == (wstats[0], wstats[1])
    assert m.group(2) == "%.4f" % wstats[2] and m.group(4) == "%.17g" % (CAPTURE_CENTER + scene["applied"])


def test_cli_save_only_chunk_and_batch(scene, cli, tmp_path):
    """--save-only: the same file and an empty stdout; --chunk 2^19 the same bytes as 2^20; two recordings with `auto` and
    --out-dir leave two files, each equal to a run of its own"""
    want, _ = sm.quantise(scene["y"], irdm.FMT_CI8, 4.0)
    only = tmp_path / "only.ci8"
    a = run_exe(cli["common"] + ["--chunk", 1 << 20, "--save-band", only, "--save-gain", 4, "--save-only"])
    assert (a.returncode, a.stdout, a.stderr) == (0, b"", b""), a.stderr.decode()[-2000:]
    assert only.read_bytes() == want
    half = tmp_path / "half.ci8"
    b = run_exe(cli["common"] + ["--chunk", 1 << 19, "--save-band", half, "--save-gain", 4])
    assert b.returncode == 0 and half.read_bytes() == want
    assert bit_fields(b.stdout) == bit_fields(cli["base"].stdout)
    # a second, shorter recording; each against a --save-only run of its own
    n2 = 20_000_000 + 1234
    short = tmp_path / "short.ci8"
    scene["x"][:2 * n2].tofile(str(short))
    own = tmp_path / "own.ci16"
    common2 = [a_ if a_ is not cli["wide"] else short for a_ in cli["common"]]
    c = run_exe(common2 + ["--save-band", own, "--save-only"])
    assert c.returncode == 0 and own.stat().st_size == 4 * ((n2 + 4) // 5)
    od = tmp_path / "od"
    two = run_exe(["-f", cli["wide"]] + common2 + ["--chunk", 1 << 20, "--out-dir", od, "--save-band", "auto", "--save-format", "ci16"])
    assert two.returncode == 0, two.stderr.decode()[-2000:]
    assert (od / "wide.ci8.band.ci16").read_bytes() == sm.quantise(scene["y"], irdm.FMT_CI16, 1.0)[0]
    assert (od / "short.ci8.band.ci16").read_bytes() == own.read_bytes()
    assert (od / "wide.ci8.out").read_bytes().count(b"RAW: ") == fm.SCENE["n_inband"]


def test_cli_usage_errors(cli, tmp_path):
    """every refusal: exit status 2, nothing on stdout, no file"""
    fe = ["--band-center", "1626000000", "--decimate", "5"]
    o = str(tmp_path / "o")
    for extra in (["--save-band", o + ".cf32"],                                         # no front end
                  fe + ["--save-band", o + ".iq"],                                      # no format by extension
                  fe + ["--save-band", o + ".ci8", "--save-format", "ci12"],
                  fe + ["--save-band", o + ".ci8", "--save-gain", "0"],
                  fe + ["--save-band", o + ".ci8", "--save-gain", "-2"],
                  fe + ["--save-band", o + ".ci8", "--save-gain", "inf"],
                  fe + ["--save-band", o + ".ci8", "--save-gain", "nan"],
                  fe + ["--save-band", o + ".ci8", "--save-gain", "x"],
                  fe + ["--save-band", o + ".cf32", "--save-gain", "2"],                # cf32 takes gain 1 only
                  fe + ["--save-only"],                                                 # needs --save-band
                  fe + ["--save-gain", "2"],
                  fe + ["--save-format", "ci8"],
                  fe + ["--save-band", o + ".ci8", "-f", str(cli["wide"])],             # several recordings want `auto`
                  fe + ["--save-band", "auto", "--save-format", "ci8"],                 # ... and --out-dir
                  fe + ["--save-band", "auto", "--out-dir", str(tmp_path / "d")]):      # ... and a named format
        r = run_exe(["-f", cli["wide"], "-r", "50000000"] + extra)
        assert r.returncode == 2 and r.stdout == b"", (extra, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def test_cli_resample_saves_the_resample_models_band(tmp_path):
    """--resample-to 10000000 --save-band out.cf32 on the head of the 11.2 MS/s scene: the resample model's bytes"""
    s = rm.SCENES["11.2->10"]
    x, _ = rm.offgrid_scene("11.2->10", irdm.FMT_CI8)
    n = (1 << 21) + 777
    x = x[:2 * n]
    cap = tmp_path / "cap.ci8"
    x.tofile(str(cap))
    cc, shift = 1621000000.0, 150_000.0
    q = fm.quantise(shift, s["in_rate"])
    want = rm.run(x, irdm.FMT_CI8, 25, 28, q, rm.design_taps(s["in_rate"], s["out_rate"]))
    out = tmp_path / "out.cf32"
    common = ["-f", cap, "-r", s["in_rate"], "-c", "%.3f" % cc, "--band-center", "%.3f" % (cc + shift), "--resample-to", s["out_rate"],
              "--chunk", 1 << 19, "--start-time", "1700000000"]
    a = run_exe(common + ["--save-band", out])
    b = run_exe(common)
    assert a.returncode == 0 and (a.stdout, a.stderr) == (b.stdout, b.stderr), a.stderr.decode()[-2000:]
    assert out.read_bytes() == want.tobytes()
    only = tmp_path / "only.ci16"
    c = run_exe(common + ["--save-band", only, "--save-only"])
    assert c.returncode == 0 and c.stdout == b"" and only.read_bytes() == sm.quantise(want, irdm.FMT_CI16, 1.0)[0]
