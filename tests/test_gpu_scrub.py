"""Option scrub on the GPU: the kernel (csrc/scrub.hpp) exact against the numpy model of tests/scrub_model.py through
irdm_scrub_device; options scrub / scrub_limit_log2 through irdm_feed_host on a scene with NaN, Inf and 1e30 written into the
gaps between its bursts, at pipeline_depth 0 and 3; irdm_frontend_scrub in front of a decimating front end that saves its
band; and the binary's --scrub."""
import functools
import os
import subprocess

import numpy as np
import pytest

import irdm
import scrub_checks as sc
import scrub_model as sm
import siggen

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(irdm.LIB_PATH), "iridium-sniffer-hip")


def test_kernel_equals_the_model():
    """n in 0 .. 5, 255 .. 257, 4095 .. 4097 and 65536 + 3, the buffer 0 and 1 sample behind a 16-byte boundary, and
    2048 x 256 + 777 pieces (the grid is capped at 2048 workgroups of 256: some lanes take a second piece); no bad sample,
    all bad, about 1 %, and single ones at the head, the tail, the edge of a wavefront and of a workgroup, in I, in Q and in
    both; quiet and signalling NaN, +-Inf and the float behind +-2^e zeroed, +-2^e, -0.0 and subnormals kept, at e = 0, 24,
    40, 127: the buffer and the guard bytes exact, all six figures exact, a second pass changes and counts nothing"""
    assert sc.kernel_cases(extra_pieces=(2048 * 256 + 777,)) > 500


def test_other_formats_and_refusals():
    """the seven formats that are not cf32: 0, the buffer untouched; -1 for an unknown format, a pointer that is not aligned
    to a sample and a limit outside 0 .. 127"""
    assert sc.refusal_cases() == 7


@pytest.mark.parametrize("depth", (0, 3))
def test_pipeline_with_scrub_equals_the_scrubbed_stream(depth):
    """a context with scrub on, fed the stream as recorded in chunks of 262 144 samples through the staging buffer
    (depth 0) and the ring slot (depth 3), yields the records of a context without it fed the model-scrubbed stream, bit for
    bit, and agrees with the oracle on that stream; irdm_scrub_stats equals the model's figures in stream coordinates;
    irdm_reset clears them; a change of either option in mid-stream and a device feed with the option on return -1"""
    res = sc.pipeline_case(depth)
    assert res["demods"] == 12 and res["frames"] == 12, res


# ---------------------------------------------------------------- the front end ----
FE = dict(fs_in=10_000_000, D=5, shift_hz=1_500_000.0)
FE_CHUNK = 1 << 18


@functools.lru_cache(maxsize=None)
def capture():
    """a 10 MS/s cf32 capture of about 0.1 s with two bursts in the band 1.5 MHz above its centre, as interleaved floats:
    as it is, with four bad samples -- the first, the last, and those on either side of the first chunk's edge --, and the
    model's scrub of that with its figures"""
    fs = FE["fs_in"]
    fe = irdm.Frontend(fs, irdm.FMT_CF32, FE["D"], FE["shift_hz"])
    applied = fe.applied_shift_hz
    fe.close()
    bursts = [dict(start=int((0.03 + 0.03 * k) * fs), freq_hz=applied + siggen.channel_freq(3 - 7 * k), payload=[k, 1, 2, 3] * 40, amp=0.05)
              for k in range(2)]
    n = 4 * FE_CHUNK - 32768 + 4321
    x = sc.as_floats(siggen.make_stream(fs, n, bursts, seed=57)[0]).copy()
    xp = x.copy()
    xp[0] = np.float32("nan")
    xp[2 * (FE_CHUNK - 1) + 1] = np.float32("inf")
    xp[2 * FE_CHUNK], xp[2 * FE_CHUNK + 1] = np.float32("-inf"), np.float32(1e30)
    xp[2 * (n - 1)] = np.float32(1e30)
    xpp, fig = sm.scrub(xp, 40)
    assert (fig["n_zeroed"], fig["n_nonfinite"], fig["n_over"], fig["first"], fig["last"]) == (4, 3, 2, 0, n - 1)
    return xp, xpp, fig, n


def front_end_run(x, scrub, depth, after=None):
    """the cf32 capture x (interleaved floats) through the front end, feed_host in chunks of 262 144 capture samples, the
    band saved as cf32"""
    fe = irdm.Frontend(FE["fs_in"], irdm.FMT_CF32, FE["D"], FE["shift_hz"])
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, center_frequency=1622000000.0 + fe.applied_shift_hz,
                      max_chunk_samples=1 << 18, max_bursts_per_chunk=256, pipeline_depth=depth)
    try:
        fe.save(irdm.FMT_CF32)
        if scrub:
            fe.scrub(True)
        c = x.view(np.complex64)
        for off in range(0, len(c), FE_CHUNK):
            fe.feed_host(p, c[off:off + FE_CHUNK])
        st = fe.scrub_stats() if scrub else None
        if after:
            after(fe, p)
        fe.flush(p)
        return dict(band=b"".join(fe.saved), n_out=p.sample_count, st=st)
    finally:
        p.close()
        fe.close()


@pytest.mark.parametrize("depth", (0, 3))
def test_front_end_scrub(depth):
    """irdm_frontend_scrub on a capture with four bad samples: the band irdm_frontend_save writes (cf32) is byte for byte the
    band of the model-scrubbed capture; the figures are the model's, in capture coordinates; a device feed and a change of
    the switch or the limit in mid-stream are refused; behind irdm_frontend_reset and irdm_frontend_seek the positions
    count from the seek"""
    xp, xpp, fig, n = capture()
    seen = {}

    def refusals(fe, p):
        L = irdm.lib()
        d = irdm.device_buffer(np.zeros(2 * 4096, np.float32))
        try:
            assert L.irdm_frontend_feed_device(fe.h, p.h, d, 4096, None) == -1
            assert L.irdm_frontend_scrub(fe.h, 0, 40) == -1 and L.irdm_frontend_scrub(fe.h, 1, 24) == -1
            assert L.irdm_frontend_scrub(fe.h, 1, 40) == 0
        finally:
            irdm.device_free(d)
        seen["refusals"] = True

    on = front_end_run(xp, True, depth, after=refusals)
    off = front_end_run(xpp, False, depth)
    st = on["st"]
    print("front end scrub stats: n %d zeroed %d nonfinite %d over %d first %d last %d" % ((int(st.n_samples),) + sc.stat_tuple(st)))
    assert seen == dict(refusals=True)
    assert (int(st.n_samples), st.limit_log2, st.active) == (n, 40, 1)
    assert sc.stat_tuple(st) == tuple(fig[f] for f in sc.FIGURES), (sc.stat_tuple(st), fig)
    assert len(on["band"]) == 8 * on["n_out"] and on["n_out"] >= n // FE["D"] - 1
    assert on["band"] == off["band"]
    assert np.isfinite(np.frombuffer(on["band"], np.float32)).all()


def test_front_end_scrub_reset_seek_and_other_formats():
    """irdm_frontend_reset clears the figures and irdm_frontend_seek moves their origin; the limit is checked; a ci8 front
    end takes the switch, launches nothing and says so"""
    xp, xpp, fig, n = capture()
    fe = irdm.Frontend(FE["fs_in"], irdm.FMT_CF32, FE["D"], FE["shift_hz"])
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, max_chunk_samples=1 << 18, max_bursts_per_chunk=256, pipeline_depth=0)
    try:
        L = irdm.lib()
        assert L.irdm_frontend_scrub_stats(fe.h, irdm.ScrubStats()) == -1           # (never switched on)
        assert L.irdm_frontend_scrub(fe.h, 1, 128) == -1 and L.irdm_frontend_scrub(fe.h, 1, -1) == -1
        fe.scrub(True, 24)
        fe.feed_host(p, xp.view(np.complex64)[:FE_CHUNK])
        want = sm.scrub(xp[:2 * FE_CHUNK], 24)[1]
        st = fe.scrub_stats()
        assert (int(st.n_samples), st.limit_log2) == (FE_CHUNK, 24) and sc.stat_tuple(st) == tuple(want[f] for f in sc.FIGURES)
        fe.reset()
        p.reset()
        st = fe.scrub_stats()
        assert (int(st.n_samples), st.limit_log2, st.active) + sc.stat_tuple(st) == (0, 24, 1, 0, 0, 0, 0, 0)
        seek = 5 * 2**32 + 1000
        fe.seek(seek)
        fe.feed_host(p, xp.view(np.complex64)[:FE_CHUNK])
        st = fe.scrub_stats()
        assert int(st.n_samples) == FE_CHUNK and (int(st.first), int(st.last)) == (seek + want["first"], seek + want["last"])
    finally:
        p.close()
        fe.close()
    fe = irdm.Frontend(FE["fs_in"], irdm.FMT_CI8, FE["D"], FE["shift_hz"])
    p = irdm.Pipeline(fe.out_rate, fmt=irdm.FMT_CF32, max_chunk_samples=1 << 18, max_bursts_per_chunk=256, pipeline_depth=0)
    try:
        fe.scrub(True)
        fe.feed_host(p, np.zeros(2 * 32768, np.int8))
        st = fe.scrub_stats()
        assert (int(st.n_samples), st.limit_log2, st.active) + sc.stat_tuple(st) == (0, 40, 0, 0, 0, 0, 0, 0)
    finally:
        p.close()
        fe.close()


# ---------------------------------------------------------------- the binary ----
START = ["--start-time", "1700000000"]
COMMON = ["-r", sc.FS, "--file-info", "scrub"] + START


def run_cli(args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=180)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("scrub")
    s, sp, spp, fig, where = sc.streams()
    out = {"dir": d}
    for name, x in (("clean", s), ("bad", sp), ("scrubbed", spp)):
        out[name] = d / (name + ".cf32")
        x.tofile(out[name])
    out["ci16"] = d / "clean.ci16"
    siggen.to_ci16(s.view(np.complex64)).tofile(out["ci16"])
    out["nan"] = d / "allnan.cf32"
    np.full(2 * 4 * 32768, np.nan, np.float32).tofile(out["nan"])
    return out


def scrub_lines(stderr):
    return [l for l in stderr.splitlines() if l.startswith("scrub:")]


def bad_line(e=40):
    s, sp, spp, fig, where = sc.streams()
    f = sm.scrub(sp, e)[1]
    return ("scrub: %d samples cf32, limit 2^%d; %d zeroed (%d non-finite, %d out-of-range components), first at sample %d (%.6f s), "
            "last at %d (%.6f s)" % (len(sp) // 2, e, f["n_zeroed"], f["n_nonfinite"], f["n_over"], f["first"], f["first"] / sc.FS,
                                     f["last"], f["last"] / sc.FS))


CLEAN_LINE = "scrub: 2000000 samples cf32, limit 2^40; none zeroed"
CI16_LINE = "scrub: ci16 samples are always finite; nothing to do"


def test_cli_scrub_prints_the_scrubbed_files_lines(files):
    """-f bad.cf32 --scrub prints the stdout of -f scrubbed.cf32 byte for byte, 12 RAW lines; without the flag the bad file
    runs through with exit code 0 (what it prints is not asserted); the scrub: line of the bad file; -v names the option once;
    --scrub=24 sets the limit; --scrub=200, --scrub=x and --gpus 2 exit with 2 and an empty stdout"""
    ref = run_cli(["-f", files["scrubbed"]] + COMMON)
    fixed = run_cli(["-f", files["bad"], "--scrub", "-v"] + COMMON)
    assert ref.returncode == fixed.returncode == 0, (ref.stderr, fixed.stderr)
    print(scrub_lines(fixed.stderr))
    assert ref.stdout.count("RAW: ") == 12 and fixed.stdout == ref.stdout
    assert scrub_lines(fixed.stderr) == [bad_line()] and scrub_lines(ref.stderr) == []
    assert fixed.stderr.count("--scrub: cf32 samples with a component that is not finite or beyond +-2^40 are zeroed") == 1
    assert "--scrub" not in ref.stderr
    low = run_cli(["-f", files["bad"], "--scrub=24"] + COMMON)
    assert low.returncode == 0 and low.stdout == ref.stdout and scrub_lines(low.stderr) == [bad_line(24)], low.stderr
    for extra in (["--scrub=200"], ["--scrub=x"], ["--scrub=-1"], ["--scrub=4.5"], ["--scrub", "--gpus", "2"]):
        r = run_cli(["-f", files["bad"]] + extra + COMMON)
        assert r.returncode == 2 and r.stdout == "" and "--scrub" in r.stderr, (extra, r.stderr)


def test_cli_scrub_lines_and_their_place(files):
    """a clean file: stdout and the rest of stderr are those of the run without the flag, the line says "none zeroed"; a
    ci16 file: "always finite"; an all-NaN file: the hint at --format; the line stands behind clock: and iq: and in front of
    input:, which describes the samples as processed; --diagnostic does not imply it; a two-file batch prints one line each"""
    base = run_cli(["-f", files["clean"]] + COMMON)
    check = run_cli(["-f", files["clean"], "--scrub"] + COMMON)
    assert base.returncode == check.returncode == 0, (base.stderr, check.stderr)
    bl, cl = base.stderr.splitlines(), check.stderr.splitlines()
    assert check.stdout == base.stdout and base.stdout.count("RAW: ") == 12 and scrub_lines(base.stderr) == []
    assert bl[-1].startswith("burst_detect: tagged ") and cl[:-1] == bl and cl[-1] == CLEAN_LINE, cl[-1]
    r = run_cli(["-f", files["ci16"], "--format", "ci16", "--scrub"] + COMMON)
    assert r.returncode == 0 and r.stdout.count("RAW: ") == 12 and r.stderr.splitlines()[-1] == CI16_LINE, r.stderr
    r = run_cli(["-f", files["nan"], "--scrub"] + COMMON)
    assert r.returncode == 0 and r.stderr.splitlines()[-1] == (
        "scrub: 131072 samples cf32, limit 2^40; 131072 zeroed (262144 non-finite, 0 out-of-range components), first at sample 0 "
        "(0.000000 s), last at 131071 (0.065535 s) -- more than 0.1 % of the recording: is this file cf32 at all? check --format"), r.stderr
    full = run_cli(["-f", files["bad"], "--scrub", "--iq-check", "--clock-check", "--input-stats"] + COMMON).stderr.splitlines()
    assert full[-4].startswith("clock: ") and full[-3].startswith("iq: ") and full[-2] == bad_line() and full[-1].startswith("input: "), full[-5:]
    assert full[-1].endswith(" nonfinite 0")
    diag = run_cli(["-f", files["clean"], "--diagnostic"] + COMMON)
    assert diag.returncode == 0 and "scrub:" not in diag.stderr
    batch = run_cli(["-f", files["clean"], "-f", files["bad"], "--scrub"] + COMMON)
    assert batch.returncode == 0 and scrub_lines(batch.stderr) == [CLEAN_LINE, bad_line()], batch.stderr


def test_cli_save_only_writes_the_scrubbed_band(files):
    """--scrub with --save-only: the band file of the bad recording is the scrubbed recording's, byte for byte, and the run
    prints the recording's scrub: line"""
    a, b = files["dir"] / "scrubbed.band.cf32", files["dir"] / "fixed.band.cf32"
    args = ["-r", "2400000", "--resample-to", "2000000", "--save-only", "--save-band"]      # (read as a 2.4 MS/s capture: 5/6)
    ra = run_cli(["-f", files["scrubbed"]] + args + [a])
    rb = run_cli(["-f", files["bad"], "--scrub"] + args + [b])
    assert ra.returncode == rb.returncode == 0, (ra.stderr, rb.stderr)
    assert a.stat().st_size > 8 * 1_000_000 and a.read_bytes() == b.read_bytes()
    s, sp, spp, fig, where = sc.streams()
    want = bad_line().replace("(%.6f s)" % (fig["last"] / sc.FS), "(%.6f s)" % (fig["last"] / 2400000.0))
    assert scrub_lines(rb.stderr) == [want] and scrub_lines(ra.stderr) == []
