"""Receiver I/Q imbalance on the GPU: the kernels of csrc/iq_balance.hpp and csrc/iq_moments.hpp against the numpy model of
tests/balance_model.py through irdm_iq_balance_device / irdm_iq_moments_device; irdm_iq_balance and option iq_moments
through irdm_feed_host on a scene with 1 dB and 5 degrees planted, at pipeline_depth 0 and 3; irdm_frontend_iq_balance and
irdm_frontend_iq_moments in front of a decimating front end that saves its band; and the binary's --image-check and
--iq-balance."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import balance_checks as bc
import balance_model as bm
import irdm
import siggen

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")
# (the grid is capped at 2048 workgroups of 256 lanes: with this many 16-byte pieces some lanes take a second one)
BIG = 2048 * 256 + 777


def test_balance_kernel_equals_the_model():
    """all eight formats, n in 0 .. 5, 255 .. 257, 4095 .. 4097, 65536 + 3 and 2048 x 256 + 777 pieces, src 0 .. 3 samples and
    dst 0 and 1 sample behind a 16-byte boundary, three coefficient pairs with the identity among them, cf32 with quiet and
    signalling NaN, +-Inf, -0.0, subnormals and products that are subnormal, and cf32 in place: every bit the model's (a NaN
    where the model has one), the guard bytes and the source untouched"""
    res = bc.balance_kernel_cases(extra_pieces=(BIG,))
    assert res["cases"] == 8 * 13 * 4 * 2 + 8 and res["in_place"] == 13 * 4 * 2 + 1, res


def test_balance_refusals():
    """an unknown format, a misaligned source or destination, overlapping buffers and coefficients out of range return -1
    and write nothing; irdm_iq_balance_coeffs equals the model at the corners of its range and refuses beyond them"""
    assert bc.balance_refusal_cases() == 8


def test_moments_kernel_equals_the_model():
    """the same sizes, source alignments and formats: counts exact, each sum within N 2^-52 sum|term| of the float64 model's,
    gain and phase within 1e-6 from 4096 samples on; non-finite samples at the head, the tail, a wavefront's edge and a
    workgroup's edge left out and counted; two launches of one buffer give identical bytes; valid = 0 for n = 0, n = 1, an
    all-zero and an all-NaN buffer"""
    res = bc.moments_kernel_cases(extra_pieces=(BIG,))
    assert res["cases"] == 8 * 13 * 4 + 8 and res["left_out"] > 100, res


@pytest.mark.parametrize("depth", (0, 3))
def test_pipeline_with_balance_equals_the_corrected_stream(depth):
    """a context with irdm_iq_balance (cf32 wire) fed the impaired stream in chunks of 262 144 samples yields the records of a
    plain context fed the model-corrected stream, bit for bit, and agrees with the oracle on that stream; option iq_moments
    on the corrected stream reads below -60 dB (model: -95); irdm_reset clears the moments and keeps the balance; a change
    of the balance after the first feed and a device feed with it on return -1"""
    res = bc.pipeline_case(depth)
    assert res["demods"] == 12 and res["frames"] == 12, res


@pytest.mark.parametrize("fmt", (irdm.FMT_CI8, irdm.FMT_CI16))
@pytest.mark.parametrize("depth", (0, 3))
def test_pipeline_with_balance_from_integer_wire_formats(depth, fmt):
    """the ci8 (scale 256) and ci16 renderings of the impaired stream as wire format, against a plain cf32 context fed the
    model's correction of their conversion: every record queue bit for bit"""
    assert bc.wire_case(depth, fmt)["demods"] >= 10


@pytest.mark.parametrize("depth", (0, 3))
def test_stream_moments_find_the_planted_imbalance(depth):
    """option iq_moments on the impaired stream: the model's figures, within 0.01 dB and 0.05 degrees of the planted 1 dB and
    5 degrees (model: 0.0009 dB and 0.008 degrees off); -1 without the option, for a member of a group, and
    irdm_iq_balance on a context that is not cf32"""
    res = bc.moments_case(depth)
    assert res["demods"] == 24, res


# ---------------------------------------------------------------- the front end ----
FE = dict(fs_in=10_000_000, D=5, shift_hz=1_500_000.0)
FE_CHUNK = 1 << 18


@functools.lru_cache(maxsize=None)
def capture():
    """a 10 MS/s cf32 capture of about 0.1 s with two bursts in the band 1.5 MHz above its centre (tests/test_gpu_scrub.py's
    shape), 1 dB and 5 degrees of imbalance planted: as interleaved floats, its ci8 rendering (scale 256), and the model's
    corrections of both"""
    fs = FE["fs_in"]
    fe = irdm.Frontend(fs, irdm.FMT_CF32, FE["D"], FE["shift_hz"])
    applied = fe.applied_shift_hz
    fe.close()
    bursts = [dict(start=int((0.03 + 0.03 * k) * fs), freq_hz=applied + siggen.channel_freq(3 - 7 * k), payload=[k, 1, 2, 3] * 40, amp=0.05)
              for k in range(2)]
    n = 4 * FE_CHUNK - 32768 + 4321
    x = bc.as_floats(siggen.make_stream(fs, n, bursts, seed=57)[0]).copy()
    y = bm.impair(x, *bc.PLANTED)
    coeffs = bm.coeffs(*bc.REMEDY)
    y8 = siggen.to_ci8(y.view(np.complex64), scale=256)
    return y, bm.balance(y, *coeffs), y8, bm.balance(bm.convert(y8, irdm.FMT_CI8), *coeffs), n


def front_end_run(x, balance, depth, after=None):
    """a capture (interleaved floats, or int8 codes with balance = ci8) through a cf32 front end, feed_host in chunks of
    262 144 capture samples, the band saved as cf32, the moments of the capture as the kernel sees it"""
    fe = irdm.Frontend(FE["fs_in"], irdm.FMT_CF32, FE["D"], FE["shift_hz"])
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, center_frequency=1622000000.0 + fe.applied_shift_hz,
                      max_chunk_samples=1 << 18, max_bursts_per_chunk=256, pipeline_depth=depth)
    try:
        fe.save(irdm.FMT_CF32)
        fe.iq_moments_enable(True)
        if balance is not None:
            fe.iq_balance(balance, *bc.REMEDY)
        for off in range(0, len(x), 2 * FE_CHUNK):
            piece = x[off:off + 2 * FE_CHUNK]
            fe.feed_host(p, piece.view(np.complex64) if piece.dtype == np.float32 else piece)
        st = fe.iq_moments()
        if after:
            after(fe, p)
        fe.flush(p)
        return dict(band=b"".join(fe.saved), n_out=p.sample_count, st=st)
    finally:
        p.close()
        fe.close()


@pytest.mark.parametrize("depth", (0, 3))
def test_front_end_balance(depth):
    """irdm_frontend_iq_balance on the impaired capture, cf32 and ci8 wire formats: the band irdm_frontend_save writes is byte
    for byte the band of the model-corrected capture; irdm_frontend_iq_moments_stats equals the model on the capture the
    kernel sees (corrected, and as recorded in a front end without the balance); a device feed and a change in mid-capture
    are refused; irdm_frontend_reset clears the moments and keeps the balance"""
    y, z, y8, z8, n = capture()
    seen = {}

    def refusals(fe, p):
        L = irdm.lib()
        d = irdm.device_buffer(np.zeros(2 * 4096, np.float32))
        try:
            assert L.irdm_frontend_feed_device(fe.h, p.h, d, 4096, None) == -1
            assert L.irdm_frontend_iq_balance(fe.h, irdm.FMT_CF32, 0.5, 1.0) == -1
        finally:
            irdm.device_free(d)
        seen["refusals"] = True

    on = front_end_run(y, irdm.FMT_CF32, depth, after=refusals)
    off = front_end_run(z, None, depth)
    assert seen == dict(refusals=True)
    assert len(on["band"]) == 8 * on["n_out"] and on["n_out"] >= n // FE["D"] - 1
    assert on["band"] == off["band"]
    mz = bm.moments(z)
    for r in (on, off):
        bc.check_moments(r["st"], mz, "front end, corrected", derived=True)
    print("front end, corrected capture: image %.1f dB" % on["st"].image_db)
    assert on["st"].image_db < -60.0
    on8 = front_end_run(y8, irdm.FMT_CI8, depth)
    off8 = front_end_run(z8, None, depth)
    assert on8["band"] == off8["band"] and len(on8["band"]) == len(on["band"])
    bc.check_moments(on8["st"], bm.moments(z8), "front end, ci8 wire", derived=True)
    raw = front_end_run(y, None, depth)
    bc.check_moments(raw["st"], bm.moments(y), "front end, as recorded", derived=True)
    assert abs(raw["st"].gain_db - bc.PLANTED[0]) <= 0.01 and abs(raw["st"].phase_deg - bc.PLANTED[1]) <= 0.05
    assert raw["band"] != on["band"]


def test_front_end_reset_and_other_formats():
    """irdm_frontend_reset clears the moments and keeps the balance; a ci8 front end refuses the balance; the figures are
    refused before the switch was ever set"""
    y, z, y8, z8, n = capture()
    fe = irdm.Frontend(FE["fs_in"], irdm.FMT_CF32, FE["D"], FE["shift_hz"])
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, max_chunk_samples=1 << 18, max_bursts_per_chunk=256, pipeline_depth=0)
    try:
        L = irdm.lib()
        assert L.irdm_frontend_iq_moments_stats(fe.h, irdm.IqMoments()) == -1
        assert L.irdm_frontend_iq_balance(fe.h, irdm.FMT_CF32, 7.0, 0.0) == -1 and L.irdm_frontend_iq_balance(fe.h, 5, 0.0, 0.0) == -1
        fe.iq_moments_enable(True)
        fe.iq_balance(irdm.FMT_CF32, *bc.REMEDY)
        fe.feed_host(p, y.view(np.complex64)[:FE_CHUNK])
        bc.check_moments(fe.iq_moments(), bm.moments(z[:2 * FE_CHUNK]), "first chunk", derived=True)
        fe.reset()
        p.reset()
        st = fe.iq_moments()
        assert (int(st.n_samples), int(st.n_used), st.valid) == (0, 0, 0)
        fe.feed_host(p, y.view(np.complex64)[:FE_CHUNK])
        bc.check_moments(fe.iq_moments(), bm.moments(z[:2 * FE_CHUNK]), "after reset", derived=True)
    finally:
        p.close()
        fe.close()
    fe = irdm.Frontend(FE["fs_in"], irdm.FMT_CI8, FE["D"], FE["shift_hz"])
    try:
        assert irdm.lib().irdm_frontend_iq_balance(fe.h, irdm.FMT_CI8, *bc.REMEDY) == -1
    finally:
        fe.close()


# ---------------------------------------------------------------- the binary ----
START = ["--start-time", "1700000000"]
COMMON = ["-r", bc.FS, "--file-info", "balance"] + START
CENTRE = 1622000000.0                                   # (the binary's default -c, and the oracle's)
FLAG = "--iq-balance=%.3f,%.2f" % bc.REMEDY


def run_cli(args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=180)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("balance")
    s, y, z = bc.streams()
    y8, z8 = bc.wire_streams(irdm.FMT_CI8)
    out = {"dir": d}
    for name, x in (("clean.cf32", s), ("impaired.cf32", y), ("corrected.cf32", z), ("impaired.ci8", y8), ("corrected8.cf32", z8)):
        out[name] = d / name
        x.tofile(out[name])
    return out


def image_lines(stderr):
    return [l for l in stderr.splitlines() if l.startswith("image:")]


def model_line(x, which, balanced=False):
    """the line the binary owes for the stream x (interleaved floats): the model's moments, the model's rule on the oracle's
    frames"""
    images, n_ok = bm.count_images(bm.frames_of(bc.oracle(which).demods), CENTRE)
    return bm.image_line(bm.moments(x), images, n_ok, balanced)


def test_cli_image_check_finds_the_imbalance_and_its_remedy_works(files):
    """-f impaired.cf32 --image-check prints 24 RAW lines and the image: line with the model's figures, the model's count on
    the oracle's frames (10 of 24) and the remedy; the flag parsed out of that line, given to a second run, prints the 12 RAW
    lines of a plain run over the model-corrected file, byte for byte, and "image below -60 dB; 0 of 12"; the same over the
    ci8 rendering equals a plain run over its model-corrected file; -v names the option once; a wrong correction is told to
    adjust it"""
    s, y, z = bc.streams()
    first = run_cli(["-f", files["impaired.cf32"], "--image-check"] + COMMON)
    assert first.returncode == 0, first.stderr
    print(image_lines(first.stderr))
    want = model_line(y, "y")
    assert first.stdout.count("RAW: ") == 24 and image_lines(first.stderr) == [want]
    assert "10 of 24 frames are images of a stronger frame -- receiver I/Q imbalance: run with " + FLAG in want
    flag = re.search(r"run with (--iq-balance=\S+)$", image_lines(first.stderr)[0]).group(1)
    assert flag == FLAG
    ref = run_cli(["-f", files["corrected.cf32"]] + COMMON)
    fixed = run_cli(["-f", files["impaired.cf32"], "--image-check", flag, "-v"] + COMMON)
    assert ref.returncode == fixed.returncode == 0, (ref.stderr, fixed.stderr)
    print(image_lines(fixed.stderr))
    assert ref.stdout.count("RAW: ") == 12 and fixed.stdout == ref.stdout
    assert image_lines(fixed.stderr) == [model_line(z, "z", balanced=True)] and image_lines(ref.stderr) == []
    assert "image below -60 dB; 0 of 12 frames are images" in image_lines(fixed.stderr)[0]
    a, b = bm.coeffs(*bc.REMEDY)
    assert fixed.stderr.count("--iq-balance: Q/I gain +0.999 dB, phase +4.99 deg: q' = %.9g i + %.9g q on the GPU, cf32 in" % (a, b)) == 1
    assert "--iq-balance" not in ref.stderr
    ref8 = run_cli(["-f", files["corrected8.cf32"]] + COMMON)
    fixed8 = run_cli(["-f", files["impaired.ci8"], "--format", "ci8", "--image-check", flag] + COMMON)
    assert ref8.returncode == fixed8.returncode == 0, (ref8.stderr, fixed8.stderr)
    assert ref8.stdout.count("RAW: ") >= 10 and fixed8.stdout == ref8.stdout
    # (8 bits at scale 256 put the noise at half an LSB, where rounding beside unequal DC offsets leaves the two arms with
    # unequal variances: the figures of that stream are the model's, not zero)
    z8 = bc.wire_streams(irdm.FMT_CI8)[1]
    assert image_lines(fixed8.stderr) == [bm.image_line(bm.moments(z8), 0, ref8.stdout.count("RAW: "), balanced=True)], fixed8.stderr
    wrong = run_cli(["-f", files["impaired.cf32"], "--image-check", "--iq-balance=0.3,1"] + COMMON)
    assert wrong.returncode == 0 and image_lines(wrong.stderr)[0].endswith(" -- receiver I/Q imbalance: with --iq-balance in effect: adjust it"), wrong.stderr


def test_cli_image_line_and_its_place(files):
    """a clean file: stdout and the rest of stderr are those of the run without the flag; the line stands behind clock: and
    iq: and in front of scrub: and input:, which describe the stream as processed (cf32 with --iq-balance); --diagnostic
    does not imply it; a two-file batch prints one line each; an empty file has nothing to judge"""
    s, y, z = bc.streams()
    base = run_cli(["-f", files["clean.cf32"]] + COMMON)
    check = run_cli(["-f", files["clean.cf32"], "--image-check"] + COMMON)
    assert base.returncode == check.returncode == 0, (base.stderr, check.stderr)
    bl, cl = base.stderr.splitlines(), check.stderr.splitlines()
    assert check.stdout == base.stdout and base.stdout.count("RAW: ") == 12 and image_lines(base.stderr) == []
    assert bl[-1].startswith("burst_detect: tagged ") and cl[:-1] == bl and cl[-1] == model_line(s, "s"), cl[-1]
    assert re.fullmatch(r"image: 2000000 samples; Q/I gain [+-]0\.00\d dB, phase [+-]0\.0\d deg: image below -60 dB; 0 of 12 frames are images", cl[-1])
    full = run_cli(["-f", files["impaired.ci8"], "--format", "ci8", "--image-check", FLAG, "--scrub", "--iq-check", "--clock-check",
                    "--input-stats"] + COMMON).stderr.splitlines()
    assert [l.split(":")[0] for l in full[-5:]] == ["clock", "iq", "image", "scrub", "input"], full[-6:]
    assert full[-2].startswith("scrub: 2000000 samples cf32, ") and full[-1].startswith("input: 2000000 samples cf32"), full[-2:]
    diag = run_cli(["-f", files["clean.cf32"], "--diagnostic"] + COMMON)
    assert diag.returncode == 0 and "image:" not in diag.stderr
    batch = run_cli(["-f", files["clean.cf32"], "-f", files["impaired.cf32"], "--image-check"] + COMMON)
    assert batch.returncode == 0 and image_lines(batch.stderr) == [model_line(s, "s"), model_line(y, "y")], batch.stderr
    empty = files["dir"] / "empty.cf32"
    empty.write_bytes(b"")
    r = run_cli(["-f", empty, "--image-check"] + COMMON)
    assert r.returncode == 0 and image_lines(r.stderr) == ["image: 0 samples; nothing to judge"], r.stderr


def test_cli_save_only_writes_the_corrected_band(files):
    """--iq-balance with --save-only: the band file of the impaired recording (cf32 and ci8) is the model-corrected
    recording's, byte for byte"""
    args = ["-r", "2400000", "--resample-to", "2000000", "--save-only", "--save-band"]      # (read as a 2.4 MS/s capture: 5/6)
    for src, ref, extra in (("impaired.cf32", "corrected.cf32", []), ("impaired.ci8", "corrected8.cf32", ["--format", "ci8"])):
        a, b = files["dir"] / (ref + ".band.cf32"), files["dir"] / (src + ".band.cf32")
        ra = run_cli(["-f", files[ref]] + args + [a])
        rb = run_cli(["-f", files[src], FLAG] + extra + args + [b])
        assert ra.returncode == rb.returncode == 0, (ra.stderr, rb.stderr)
        assert a.stat().st_size > 8 * 1_000_000 and a.read_bytes() == b.read_bytes(), src
    plain = files["dir"] / "plain.band.cf32"
    assert run_cli(["-f", files["impaired.cf32"]] + args + [plain]).returncode == 0
    assert plain.read_bytes() != (files["dir"] / "impaired.cf32.band.cf32").read_bytes()


def test_cli_refusals(files):
    """--gpus 2 with either flag, --image-check with --save-only, figures outside +-6 dB / +-30 degrees and anything that is
    not two numbers exit with 2 and an empty stdout"""
    save = ["-r", "2400000", "--resample-to", "2000000", "--save-only", "--save-band", files["dir"] / "never.cf32"]
    for extra in (["--image-check", "--gpus", "2"], [FLAG, "--gpus", "2"], ["--iq-balance=6.5,0"], ["--iq-balance=0,-30.5"],
                  ["--iq-balance=1"], ["--iq-balance=1,"], ["--iq-balance=,1"], ["--iq-balance=a,b"], ["--iq-balance=1,2,3"],
                  ["--iq-balance=1,2x"], ["--iq-balance=nan,0"], ["--iq-balance="], ["--iq-balance"]):
        r = run_cli(["-f", files["clean.cf32"]] + extra + COMMON)
        assert r.returncode == 2 and r.stdout == "" and ("--iq-balance" in r.stderr or "--image-check" in r.stderr), (extra, r.stderr)
    r = run_cli(["-f", files["clean.cf32"], "--image-check"] + save)
    assert r.returncode == 2 and r.stdout == "" and "--image-check" in r.stderr, r.stderr
    assert not (files["dir"] / "never.cf32").exists()
